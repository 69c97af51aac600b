// tests/hipemu/emu_entropy_segments.cpp -- TEST INFRASTRUCTURE ONLY.
// The GPU entropy stage (cineform-sdk_amd/csrc/cfhd_entropy_kernels.h, unmodified source) under the CPU emulation of tests/hipemu, with the level-1 segment length
// and the count kernel chosen by the caller: k_ent_count over the dense bands, or k_ent_count_blocks over block lists built here from the same coefficients (the form
// cfhd_kernels.h FwdBlockLists describes).  tests/test_entropy_long_segments.py checks that every choice writes the same sample.
#include "hip_emu.h"
#define CFHD_ENT_FILL 64          // k_ent_layout: pieces of 16 words, so that the small test frames give holes of many pieces
dim3 threadIdx, blockIdx, blockDim, gridDim;
#include "cfhd_entropy_jobs.h"
#include <vector>

// count_mode 0: k_ent_count over every band; 1: the level-1 bands through k_ent_count_blocks.  stats (may be null): [0] segments, [1] level-1 segments longer than
// dev::ENT_SEG, [2] segments whose bits do not fit k_ent_emit's LDS window, [3] the most bits of any segment, [4] the segments' token slots.
extern "C" long emu_entropy_encode_segments(int width, int height, int pixel_kind, int quality, unsigned frame_number, int16_t *coeffs, const uint8_t *meta, size_t meta_size,
                                            uint8_t *out, size_t cap, int interlaced, int l1_seg, int count_mode, long *stats)
{
	using namespace cfhd;
	FramePlan plan;
	if (!build_frame_plan(&plan, width, height, pixel_kind, ENC_YUV422)) return -1;
	plan.interlaced = interlaced != 0;
	if (count_mode && plan.interlaced) return -5;        // (no block lists for interlaced frames)
	QuantState st = {0, -1, 0};
	derive_quantization(&plan, quality, !interlaced, 0.0f, &st);
	SampleHeaderInfo hdr = { frame_number, pixel_kind == PIX_2VUY ? 1 : 2, 2, quality, !interlaced, meta, meta_size, nullptr, 0 };
	SampleTemplate t;
	build_sample_template(plan, hdr, &t);
	EntHostJobs jobs;
	if (!ent_build_band_jobs(plan, t, 1, coeffs, plan.coeff_elems, &jobs, l1_seg)) return -2;
	std::vector<uint8_t> block(kEntTmplStride, 0);
	if (!ent_fill_frame_block(plan, t, 0, jobs, coeffs, block.data())) return -3;
	uint32_t size = 0, peak_flag = 0;
	dev::EntFrameJob fj = ent_frame_job(t, block.data(), out, (uint32_t)cap, &size, &peak_flag);
	static dev::EntTables tables[2]; static bool ready = false;
	if (!ready) { ent_build_tables(&tables[0], 1); ent_build_tables(&tables[1], 2); ready = true; }
	const int nseg = (int)jobs.segjobs.size(), nb = (int)jobs.bands.size();
	std::vector<dev::EntSegState> segs(nseg);
	std::vector<dev::EntBandState> bstate(nb);
	const dev::EntBatchGeom geom = { nseg, nb, 0, jobs.tok_per_frame };
	std::vector<uint32_t> tokens(jobs.tok_per_frame, 0xdeadbeefu);
	// block lists of the level-1 bands: per band row, chunks of 62 blocks of 8; a block with a nonzero coefficient is listed -- its bit in the chunk's mask, its
	// coefficients at the chunk's next free slot in the band's own block slots (the slot array mirrors the pyramid: slot = coefficient offset / 8)
	int mask_base[kMaxChannels][kNumBands];
	const int nmasks = block_list_layout(plan, mask_base);
	std::vector<uint4> blocks(plan.coeff_elems / 8 + 1);
	std::vector<unsigned long long> masks(nmasks + 1, 0ull);
	for (int c = 0; c < plan.num_channels; c++)
		for (int b = 1; b < kNumBands; b++) {
			const BandDesc &bd = plan.ch[c].band[0][b];
			const int cpr = (bd.pitch + kBlockChunkCols - 1) / kBlockChunkCols;
			for (int r = 0; r < bd.height; r++)
				for (int k = 0; k < cpr; k++) {
					unsigned long long m = 0; int rank = 0;
					for (int i = 0; i < kBlockChunkCols / 8 && k * kBlockChunkCols + 8 * i < bd.pitch; i++) {
						const int16_t *src = coeffs + bd.offset + (size_t)r * bd.pitch + k * kBlockChunkCols + 8 * i;
						bool any = false;
						for (int e = 0; e < 8; e++) any |= src[e] != 0;
						if (!any) continue;
						m |= 1ull << i;
						memcpy(&blocks[(bd.offset + (size_t)r * bd.pitch) / 8 + (size_t)k * (kBlockChunkCols / 8) + rank++], src, 16);
					}
					masks[mask_base[c][b] + r * cpr + k] = m;
				}
		}
	const dev::EntBlockLists lists = { blocks.data(), masks.data(), coeffs, (size_t)nmasks };
	auto count = [&](int lo, int n, bool level1) {
		const unsigned grid = (unsigned)((n + dev::ENT_WAVES - 1) / dev::ENT_WAVES);
		if (level1 && count_mode) hipemu::launch(dim3(grid), dim3(dev::ENT_THREADS), [&] { dev::k_ent_count_blocks(jobs.segjobs.data(), geom, n, segs.data(), tables, &peak_flag, tokens.data(), lo, n, lists); });
		else hipemu::launch(dim3(grid), dim3(dev::ENT_THREADS), [&] { dev::k_ent_count(jobs.segjobs.data(), geom, n, segs.data(), tables, &peak_flag, tokens.data(), lo, n); });
	};
	for (const auto &r : jobs.ranges_l1) count(r.first, r.second, true);
	for (const auto &r : jobs.ranges_rest) count(r.first, r.second, false);
	hipemu::launch(dim3(nb), dim3(dev::ENT_THREADS), [&] { dev::k_ent_scan(jobs.bands.data(), segs.data(), bstate.data(), tables); });
	hipemu::launch(dim3(1, 3), dim3(dev::ENT_THREADS), [&] { dev::k_ent_layout(&fj, jobs.bands.data(), segs.data(), bstate.data(), tables); });
	{
		dev::EntPeakHoles which; which.n = 0;
		for (size_t h = 0; h < t.holes.size() && which.n < 7; h++) if (t.holes[h].kind == 2) which.hole[which.n++] = (int)h;
		if (which.n) hipemu::launch(dim3(2, (unsigned)which.n, 1), dim3(dev::ENT_THREADS), [&] { dev::k_ent_peaks(&fj, which, jobs.bands.data(), jobs.segjobs.data(), geom, segs.data(), bstate.data()); });
	}
	hipemu::launch(dim3((nseg + dev::ENT_WAVES - 1) / dev::ENT_WAVES), dim3(dev::ENT_THREADS), [&] { dev::k_ent_emit(nseg, segs.data(), tables, tokens.data()); });
	if (stats) {
		long nlong = 0, nwide = 0, maxbits = 0;
		for (int s = 0; s < nseg; s++) {
			if (jobs.segjobs[s].len > dev::ENT_SEG) nlong++;
			const dev::EntSegState &x = segs[s];
			if (x.bits && ((x.bitoff + x.bits - 1u) >> 5) - (x.bitoff >> 5) + 1u > (uint32_t)dev::ENT_LDS_WORDS) nwide++;
			if ((long)x.bits > maxbits) maxbits = (long)x.bits;
		}
		stats[0] = nseg; stats[1] = nlong; stats[2] = nwide; stats[3] = maxbits; stats[4] = (long)jobs.tok_per_frame;
	}
	return (peak_flag & 2u) ? -100 : (long)size;
}
