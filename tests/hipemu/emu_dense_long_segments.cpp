// tests/hipemu/emu_dense_long_segments.cpp -- TEST INFRASTRUCTURE ONLY.
// The GPU entropy stage (cineform-sdk_amd/csrc/cfhd_entropy_kernels.h, unmodified source) under the CPU emulation of tests/hipemu, with the segment length of every
// family of bands chosen by the caller (cfhd_entropy_jobs.h EntSegRule: level 1 counted densely, level 2, level 3; l1_seg: level 1 from block lists) and any input the
// frame plan serves (YUY2 / 2vuy 4:2:2, RG48 4:4:4, ...).  tests/test_entropy_dense_long_segments.py checks that every choice writes the same sample.
#include "hip_emu.h"
#define CFHD_ENT_FILL 64          // k_ent_layout: pieces of 16 words, so that the small test frames give holes of many pieces
dim3 threadIdx, blockIdx, blockDim, gridDim;
#include "cfhd_entropy_jobs.h"
#include <vector>

// lens: l1_seg (level 1 from block lists, when use_lists), level 1 dense, level 2, level 3.  use_lists: the level-1 bands through k_ent_count_blocks over block lists built
// here (progressive 4:2:2 only), as the product counts them at widths that are multiples of 32.
// stats (may be null): [0] segments, [1] segments longer than dev::ENT_SEG, [2] segments whose bits do not fit k_ent_emit's LDS window (ent_ordinary() false for width),
// [3] the most bits of any segment, [4] segments of bands coded with table 1, [5] the longest of those, [6] segments of [2] outside the level-1 bands that are longer
// than dev::ENT_SEG, [7] the longest segment of the level-2 / level-3 bands, [8] the longest dense level-1 segment coded with table 0.
extern "C" long emu_dense_long_encode(int width, int height, int pixel_kind, int encoded_format, int quality, int input_format, int color_space, unsigned frame_number, int16_t *coeffs,
                                      const uint8_t *meta, size_t meta_size, uint8_t *out, size_t cap, int interlaced, const int *lens, int use_lists, long *stats)
{
	using namespace cfhd;
	FramePlan plan;
	if (!build_frame_plan(&plan, width, height, pixel_kind, encoded_format)) return -1;
	plan.interlaced = interlaced != 0;
	if (use_lists && (plan.interlaced || encoded_format != ENC_YUV422)) return -5;        // (block lists: progressive 4:2:2 frames only)
	QuantState st = {0, -1, 0};
	derive_quantization(&plan, quality, !interlaced, 0.0f, &st);
	SampleHeaderInfo hdr = { frame_number, input_format, color_space, quality, !interlaced, meta, meta_size, nullptr, 0 };
	SampleTemplate t;
	build_sample_template(plan, hdr, &t);
	EntHostJobs jobs;
	const EntSegRule rule = { lens[1], lens[2], lens[3], use_lists != 0 };
	if (!ent_build_band_jobs(plan, t, 1, coeffs, plan.coeff_elems, &jobs, use_lists ? lens[0] : (int)dev::ENT_SEG, &rule)) return -2;
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
	// block lists of the level-1 bands (cfhd_kernels.h FwdBlockLists), as tests/hipemu/emu_entropy_segments.cpp builds them
	int mask_base[kMaxChannels][kNumBands];
	const int nmasks = use_lists ? block_list_layout(plan, mask_base) : 0;
	std::vector<uint4> blocks(use_lists ? plan.coeff_elems / 8 + 1 : 1);
	std::vector<unsigned long long> masks(nmasks + 1, 0ull);
	if (use_lists) for (int c = 0; c < plan.num_channels; c++)
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
		if (level1 && use_lists) hipemu::launch(dim3(grid), dim3(dev::ENT_THREADS), [&] { dev::k_ent_count_blocks(jobs.segjobs.data(), geom, n, segs.data(), tables, &peak_flag, tokens.data(), lo, n, lists); });
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
		for (int k = 0; k < 9; k++) stats[k] = 0;
		std::vector<char> rest(nseg, 0);
		for (const auto &r : jobs.ranges_rest) for (int s = r.first; s < r.first + r.second; s++) rest[s] = 1;
		for (int s = 0; s < nseg; s++) {
			const dev::EntSegJob &j = jobs.segjobs[s];
			const dev::EntSegState &x = segs[s];
			const bool wide = x.bits && ((x.bitoff + x.bits - 1u) >> 5) - (x.bitoff >> 5) + 1u > (uint32_t)dev::ENT_LDS_WORDS;
			if (j.len > dev::ENT_SEG) stats[1]++;
			if (wide) stats[2]++;
			if ((long)x.bits > stats[3]) stats[3] = (long)x.bits;
			if (j.table) { stats[4]++; if (j.len > stats[5]) stats[5] = j.len; }
			if (wide && rest[s] && j.len > dev::ENT_SEG) stats[6]++;
			if (rest[s] && j.len > stats[7]) stats[7] = j.len;
			if (!rest[s] && !j.table && !(use_lists && j.mask_base >= 0) && j.len > stats[8]) stats[8] = j.len;
		}
		stats[0] = nseg;
	}
	return (peak_flag & 2u) ? -100 : (long)size;
}
