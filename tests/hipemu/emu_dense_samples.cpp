// tests/hipemu/emu_dense_samples.cpp -- TEST INFRASTRUCTURE ONLY.
// A batch of frames through the GPU entropy stage (cineform-sdk_amd/csrc/cfhd_entropy_kernels.h, unmodified source) under the CPU emulation of tests/hipemu, the way
// GpuEntropyEncoder::launch() queues it: count, scan, k_ent_sizes + k_ent_pack_offsets, then k_ent_layout and k_ent_emit writing every sample at its offset of ONE dense
// buffer.  Geometries whose width is a multiple of 32 count their level-1 bands from block lists with long segments (k_ent_count_blocks), the others densely.
// tests/test_dense_samples_emulated.py compares sizes, offsets and bytes with the host writer.
#include "hip_emu.h"
#define CFHD_ENT_FILL 64          // k_ent_layout: pieces of 16 words, so that the small test frames give holes of many pieces
dim3 threadIdx, blockIdx, blockDim, gridDim;
#include "cfhd_entropy_jobs.h"
#include <vector>

// coeffs: nframes pyramids (product layout), plan.coeff_elems apart.  packed: the dense buffer (packed_cap bytes, 64-byte aligned); cap: what one sample may take (a
// larger one reports size 0 and takes no room).  sizes[nframes], offsets[nframes + 1]: as the device leaves them.  stats (may be null): [0] segments of the batch,
// [1] those whose bits do not fit k_ent_emit's LDS window, [2] 1 when the level-1 bands were counted from block lists.  Returns 0, or < 0.
extern "C" long emu_dense_encode(int width, int height, int pixel_kind, int quality, int nframes, int16_t *coeffs, const uint8_t *meta, size_t meta_size,
                                 uint8_t *packed, size_t packed_cap, unsigned cap, uint32_t *sizes, uint32_t *offsets, int interlaced, int layout_parts, long *stats)
{
	using namespace cfhd;
	FramePlan plan;
	if (!build_frame_plan(&plan, width, height, pixel_kind, ENC_YUV422)) return -1;
	plan.interlaced = interlaced != 0;
	if (((uintptr_t)packed & 63) || nframes < 1) return -6;
	// every sample fits cap and offsets are rounded up to 64 bytes: the dense buffer never needs more than this
	if ((((size_t)cap + 63) & ~(size_t)63) * (size_t)nframes > packed_cap) return -7;
	QuantState st = {0, -1, 0};
	derive_quantization(&plan, quality, !interlaced, 0.0f, &st);
	const bool lists_on = !plan.interlaced && plan.width % 32 == 0;
	std::vector<SampleTemplate> tmpl(nframes);
	for (int f = 0; f < nframes; f++) {
		SampleHeaderInfo hdr = { (uint32_t)f + 1, pixel_kind == PIX_2VUY ? 1 : 2, 2, quality, !interlaced, meta, meta_size, nullptr, 0 };
		build_sample_template(plan, hdr, &tmpl[f]);
	}
	EntHostJobs jobs;
	const size_t stride = plan.coeff_elems;
	if (!ent_build_band_jobs(plan, tmpl[0], nframes, coeffs, stride, &jobs, lists_on ? (int)dev::ENT_SEG_L1 : (int)dev::ENT_SEG)) return -2;
	std::vector<uint8_t> blocks_of_frames((size_t)kEntTmplStride * nframes, 0);
	std::vector<uint32_t> peak_flags(nframes, 0);
	std::vector<dev::EntFrameJob> fj(nframes);
	for (int f = 0; f < nframes; f++) {
		uint8_t *block = blocks_of_frames.data() + (size_t)kEntTmplStride * f;
		if (!ent_fill_frame_block(plan, tmpl[f], f, jobs, coeffs + stride * f, block)) return -3;
		fj[f] = ent_frame_job(tmpl[f], block, packed, cap, sizes + f, &peak_flags[f], offsets + f);
	}
	static dev::EntTables tables[2]; static bool ready = false;
	if (!ready) { ent_build_tables(&tables[0], 1); ent_build_tables(&tables[1], 2); ready = true; }
	const int total_segs = (int)jobs.segjobs.size(), per_frame = total_segs / nframes, nb = (int)jobs.bands.size();
	std::vector<dev::EntSegState> segs(total_segs);
	std::vector<dev::EntBandState> bstate(nb);
	const dev::EntBatchGeom geom = { per_frame, jobs.nbands, stride, jobs.tok_per_frame };
	std::vector<uint32_t> tokens(jobs.tok_per_frame * (size_t)nframes, 0xdeadbeefu);
	// block lists of the level-1 bands (cfhd_kernels.h FwdBlockLists), built from the dense coefficients: slots numbered over the whole batch's pyramids, masks per frame
	int mask_base[kMaxChannels][kNumBands];
	const int nmasks = block_list_layout(plan, mask_base);
	std::vector<uint4> blocks(lists_on ? stride * nframes / 8 + 1 : 1);
	std::vector<unsigned long long> masks(lists_on ? (size_t)nmasks * nframes + 1 : 1, 0ull);
	if (lists_on) for (int f = 0; f < nframes; f++)
		for (int c = 0; c < plan.num_channels; c++)
			for (int b = 1; b < kNumBands; b++) {
				const BandDesc &bd = plan.ch[c].band[0][b];
				const int cpr = (bd.pitch + kBlockChunkCols - 1) / kBlockChunkCols;
				for (int r = 0; r < bd.height; r++)
					for (int k = 0; k < cpr; k++) {
						unsigned long long m = 0; int rank = 0;
						for (int i = 0; i < kBlockChunkCols / 8 && k * kBlockChunkCols + 8 * i < bd.pitch; i++) {
							const size_t at = stride * f + bd.offset + (size_t)r * bd.pitch + k * kBlockChunkCols + 8 * i;
							bool any = false;
							for (int e = 0; e < 8; e++) any |= coeffs[at + e] != 0;
							if (!any) continue;
							m |= 1ull << i;
							memcpy(&blocks[(stride * f + bd.offset + (size_t)r * bd.pitch) / 8 + (size_t)k * (kBlockChunkCols / 8) + rank++], coeffs + at, 16);
						}
						masks[(size_t)nmasks * f + mask_base[c][b] + r * cpr + k] = m;
					}
			}
	const dev::EntBlockLists lists = { blocks.data(), masks.data(), coeffs, (size_t)nmasks };
	auto count = [&](int lo, int n, bool level1) {
		const int total = n * nframes;
		const unsigned grid = (unsigned)((total + dev::ENT_WAVES - 1) / dev::ENT_WAVES);
		if (level1 && lists_on) hipemu::launch(dim3(grid), dim3(dev::ENT_THREADS), [&] { dev::k_ent_count_blocks(jobs.segjobs.data(), geom, total, segs.data(), tables, peak_flags.data(), tokens.data(), lo, n, lists); });
		else hipemu::launch(dim3(grid), dim3(dev::ENT_THREADS), [&] { dev::k_ent_count(jobs.segjobs.data(), geom, total, segs.data(), tables, peak_flags.data(), tokens.data(), lo, n); });
	};
	for (const auto &r : jobs.ranges_l1) count(r.first, r.second, true);
	for (const auto &r : jobs.ranges_rest) count(r.first, r.second, false);
	hipemu::launch(dim3(nb), dim3(dev::ENT_THREADS), [&] { dev::k_ent_scan(jobs.bands.data(), segs.data(), bstate.data(), tables); });
	hipemu::launch(dim3((nframes + dev::ENT_WAVES - 1) / dev::ENT_WAVES), dim3(dev::ENT_THREADS), [&] { dev::k_ent_sizes(fj.data(), nframes, bstate.data()); });
	hipemu::launch(dim3(1), dim3(dev::ENT_THREADS), [&] { dev::k_ent_pack_offsets(sizes, nframes, offsets); });
	hipemu::launch(dim3(nframes, layout_parts), dim3(dev::ENT_THREADS), [&] { dev::k_ent_layout(fj.data(), jobs.bands.data(), segs.data(), bstate.data(), tables); });
	{
		dev::EntPeakHoles which; which.n = 0;
		for (size_t h = 0; h < tmpl[0].holes.size() && which.n < 7; h++) if (tmpl[0].holes[h].kind == 2) which.hole[which.n++] = (int)h;
		if (which.n) hipemu::launch(dim3(2, (unsigned)which.n, (unsigned)nframes), dim3(dev::ENT_THREADS), [&] { dev::k_ent_peaks(fj.data(), which, jobs.bands.data(), jobs.segjobs.data(), geom, segs.data(), bstate.data()); });
	}
	hipemu::launch(dim3((total_segs + dev::ENT_WAVES * dev::ENT_EMIT_SEGS - 1) / (dev::ENT_WAVES * dev::ENT_EMIT_SEGS)), dim3(dev::ENT_THREADS), [&] { dev::k_ent_emit(total_segs, segs.data(), tables, tokens.data()); });
	if (stats) {
		long nwide = 0;
		for (int s = 0; s < total_segs; s++) {
			const dev::EntSegState &x = segs[s];
			if (x.bits && ((x.bitoff + x.bits - 1u) >> 5) - (x.bitoff >> 5) + 1u > (uint32_t)dev::ENT_LDS_WORDS) nwide++;
		}
		stats[0] = total_segs; stats[1] = nwide; stats[2] = lists_on ? 1 : 0;
	}
	for (int f = 0; f < nframes; f++) if (peak_flags[f] & 2u) return -100;
	return 0;
}
