// tests/hipemu/dense_samples_asan_main.cpp -- TEST INFRASTRUCTURE ONLY.
// Stand-alone driver of emu_dense_encode() (emu_dense_samples.cpp) for a build with -fsanitize=address,undefined: batches of synthetic pyramids -- empty, sparse, dense
// noise with large values, sparse again -- through the emulated entropy stage into heap buffers of exactly the size the encoder's arithmetic promises, with and without
// a frame that exceeds the capacity.  Checks sizes and offsets against the same arithmetic on the host and parses every sample with the product's host parser.
#include "cfhd_core.h"
#include "cfhd_bitstream.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" long emu_dense_encode(int width, int height, int pixel_kind, int quality, int nframes, int16_t *coeffs, const uint8_t *meta, size_t meta_size,
                                 uint8_t *packed, size_t packed_cap, unsigned cap, uint32_t *sizes, uint32_t *offsets, int interlaced, int layout_parts, long *stats);

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int fail(const char *what, int a, long b) { printf("FAILED: %s (%d, %ld)\n", what, a, b); return 1; }

static int run(int w, int h, int interlaced)
{
	using namespace cfhd;
	FramePlan plan;
	if (!build_frame_plan(&plan, w, h, PIX_YUY2, ENC_YUV422)) return fail("plan", w, h);
	const int n = 4;
	const size_t stride = plan.coeff_elems;
	std::vector<int16_t> coeffs(stride * n, 0);
	for (int f = 0; f < n; f++)
		for (int c = 0; c < plan.num_channels; c++)
			for (int lv = 0; lv < kNumLevels; lv++)
				for (int b = lv == kNumLevels - 1 ? 0 : 1; b < kNumBands; b++) {
					const BandDesc &bd = plan.ch[c].band[lv][b];
					for (int r = 0; r < bd.height; r++)
						for (int x = 0; x < bd.width; x++) {
							int v = 0;
							if (b == 0) v = (int)(rnd() % 4000);
							else if (f == 1 || f == 3) v = rnd() % 37 == 0 ? (int)(rnd() % 9) - 4 : 0;
							else if (f == 2) v = (int)(rnd() % 1801) - 900;
							coeffs[stride * f + bd.offset + (size_t)r * bd.pitch + x] = (int16_t)v;
						}
				}
	static const uint8_t meta[24] = { 'G', 'U', 'I', 'D', 16, 0, 0, 'G', 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 };
	uint32_t full[n] = { 0, 0, 0, 0 };
	for (int pass = 0; pass < 2; pass++) {
		// pass 0: room for everything; pass 1: a capacity between the dense frame's size and the others'
		uint32_t cap = ((uint32_t)(w * h * 8 + 65536) + 255u) & ~255u;
		if (pass == 1) { uint32_t m = 0; for (int f = 0; f < n; f++) if (f != 2 && full[f] > m) m = full[f]; if (m >= full[2]) return fail("sizes too close", (int)m, (long)full[2]); cap = m; }
		const size_t room = (((size_t)cap + 63) & ~(size_t)63) * n;
		uint8_t *packed = (uint8_t *)aligned_alloc(64, room);
		uint32_t *sizes = (uint32_t *)malloc(sizeof(uint32_t) * n), *offsets = (uint32_t *)malloc(sizeof(uint32_t) * (n + 1));
		std::vector<int16_t> c2(coeffs);
		const long rc = emu_dense_encode(w, h, PIX_YUY2, 4, n, c2.data(), meta, sizeof(meta), packed, room, cap, sizes, offsets, interlaced, 3, nullptr);
		if (rc) return fail("emu_dense_encode", pass, rc);
		uint64_t at = 0;
		for (int f = 0; f < n; f++) {
			if (offsets[f] != at || (at & 63)) return fail("offset", f, (long)offsets[f]);
			if (pass == 0) full[f] = sizes[f];
			const uint32_t want = pass == 1 && f == 2 ? 0u : full[f];
			if (sizes[f] != want || sizes[f] > cap) return fail("size", f, (long)sizes[f]);
			if (sizes[f]) {
				ParsedSample ps;
				if (parse_sample(packed + at, sizes[f], &ps) != 0 || ps.width != w) return fail("parse", f, (long)sizes[f]);
			}
			at += ((uint64_t)sizes[f] + 63u) & ~(uint64_t)63u;
			if (at > room) return fail("room", f, (long)at);
		}
		if (offsets[n] != at) return fail("total", n, (long)offsets[n]);
		if (pass == 0 && (full[0] == 0 || full[2] < 4 * full[0])) return fail("sizes", (int)full[0], (long)full[2]);
		free(packed); free(sizes); free(offsets);
	}
	return 0;
}

int main()
{
	if (run(256, 144, 0) || run(176, 96, 0) || run(176, 96, 1)) return 1;
	printf("dense samples ok\n");
	return 0;
}
