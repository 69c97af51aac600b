// cfhd_thumbnail_kernels.h -- k_dec_thumbnail, the one kernel of a thumbnail pass of the decode queue (cfhd_amd_decode_batch_create_thumbnails, cfhd_decode_queue.hip)
// that is not shared with the decode passes: behind k_dec_ingest and k_dec_parse, the 1/8 x 1/8 picture of every sample straight from the raw level-3 lowpass words
// in its slot -- what CFHD_GetThumbnail writes (cfhd_api_decoder.inc thumbnail_from_sample, after Codec/thumbnail.c:65): 10-bit RGB, one big-endian longword a pixel,
// r << 22 | g << 12 | b << 2 ("DPX0").  No entropy decoder, no inverse transform, no coefficient memory.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <cfhd_gfx950.h>
#include "cfhd_lowpass_job.h"

namespace cfhd {
namespace dev {

// ---------------------------------------------------------------------------------------------
// k_dec_thumbnail: picture i of the pass, width x height pixels (width even), into pictures + i * picture_bytes -- 4 x width x height bytes, nothing behind them.
// Input: the DecLowpassJobs k_dec_parse wrote for sample i (jobs[i * nch + c], c = 0 .. 2; a fourth channel is not read), its verdict word and k_dec_ingest's mark.
// A sample whose verdict's low byte is not 0, that was not placed, or whose three lowpass bands are not width x height (4:2:2: the chroma bands width / 2 x height)
// gets zeros: no load of its slot, and no separate blanking launch.  The scan flag and the colour-space tag above the low byte play no part (the reference uses the
// one matrix whatever the sample says).
//   w is the big-endian word as stored; of it (w >> 4) & 0x3ff counts, the bits above the ten are dropped by the mask (the lowpass bias of k_dec_lowpass has no part).
//   4:2:2 (yuv422 != 0): per pixel pair, y = v(channel 0) - 64 for each pixel, cr = v(channel 1) - 512, cb = v(channel 2) - 512 for both;
//     r = clamp((1192 y + 1836 cr) >> 10), g = clamp((1192 y - 547 cr - 218 cb) >> 10), b = clamp((1192 y + 2166 cb) >> 10), clamp to 0 .. 1023; 32-bit integers,
//     arithmetic shifts, no float.
//   RGB 4:4:4 and RGBA 4:4:4:4: g, r, b = v of channels 0, 1, 2.
// The lowpass words of a channel start on a longword boundary of the 256-byte aligned slot and its rows follow each other without padding, so the picture is one run
// of width x height pixels: channel 0 one run of words, each chroma channel one run (4:2:2: a word per pixel pair).  The rows themselves start off 16-byte
// boundaries unless width is a multiple of 8 (4:2:2 chroma rows off longword boundaries when width / 2 is odd): nothing here goes row by row.
//   A lane takes DEC_THUMB_PIXELS = 8 consecutive pixels of the run: 16 bytes of channel 0 and 8 bytes of each chroma channel (RGB: 16 bytes of each), in one load
//   where the run starts on such a boundary in the slot, longword by longword where it does not (the same for every lane of the sample: a wave-uniform choice; every
//   address is a multiple of 4).  It writes 32 consecutive bytes: two 16-byte stores where the picture starts on a 16-byte boundary -- the two store instructions of a
//   wave cover 2 KB of the picture without a gap --, four 8-byte stores where it does not (4 x width x height is a multiple of 8, of 16 only when the pixel count is a
//   multiple of 4: every second picture of such a batch).  The pixels behind the last whole group of eight (2, 4 or 6: the count is even) go pair by pair, a lane each:
//   4-byte loads of channel 0, 2-byte loads of the chroma words, one 8-byte store.
//   Bounds: a group reads bytes [16 g, 16 g + 16) of a run of 2 x width x height bytes and [8 g, 8 g + 8) of one of width x height, a pair its own words; the parser
//   admitted the job only with width x height words inside the sample (cfhd_entropy_kernels.h k_dec_parse: pos + bytes <= end <= size), and this kernel takes the job
//   only with the batch's width and height.  A group writes bytes [32 g, 32 g + 32), g < width x height / 8.
// wave64, no LDS, no scratch.  Grid (pieces: dec_thumbnail_pieces(width x height), pictures), DEC_THUMB_THREADS x 8 pixels per piece and step.
// ---------------------------------------------------------------------------------------------
enum { DEC_THUMB_THREADS = 256, DEC_THUMB_PIXELS = 8, DEC_THUMB_SPLIT = 2 };
inline unsigned dec_thumbnail_pieces(int pixels)
{
	const int step = DEC_THUMB_THREADS * DEC_THUMB_PIXELS, p = (pixels + step - 1) / step;
	return (unsigned)(p < 1 ? 1 : (p > DEC_THUMB_SPLIT ? DEC_THUMB_SPLIT : p));
}

// the ten bits that count of the first and of the second big-endian word of a longword as it was loaded (v_perm_b32 swaps the bytes and clears the other half)
__device__ __forceinline__ int thumb_first10(uint32_t l) { return (int)((byte_perm(0u, l, 0x0c0c0001u) >> 4) & 0x3ffu); }
__device__ __forceinline__ int thumb_second10(uint32_t l) { return (int)((byte_perm(0u, l, 0x0c0c0203u) >> 4) & 0x3ffu); }
__device__ __forceinline__ int thumb_clamp10(int v) { return v < 0 ? 0 : (v > 0x3ff ? 0x3ff : v); }
// the DPX0 longword as the store writes it: big-endian
__device__ __forceinline__ uint32_t thumb_dpx0(int r, int g, int b) { return byte_perm(0u, ((uint32_t)r << 22) | ((uint32_t)g << 12) | ((uint32_t)b << 2), 0x00010203u); }
__device__ __forceinline__ uint32_t thumb_yuv(int y, int cr, int cb)
{
	return thumb_dpx0(thumb_clamp10((1192 * y + 1836 * cr) >> 10), thumb_clamp10((1192 * y - 547 * cr - 218 * cb) >> 10), thumb_clamp10((1192 * y + 2166 * cb) >> 10));
}
// 16 and 8 bytes at p (a multiple of 4): one load where p is a multiple of the size (wide), longwords otherwise
__device__ __forceinline__ void thumb_load16(const uint8_t *p, bool wide, uint32_t *w)
{
	if (wide) { const cfhd_u4 v = CFHD_LDG128(p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
	else { w[0] = CFHD_LDG32(p); w[1] = CFHD_LDG32(p + 4); w[2] = CFHD_LDG32(p + 8); w[3] = CFHD_LDG32(p + 12); }
}
__device__ __forceinline__ void thumb_load8(const uint8_t *p, bool wide, uint32_t *w)
{
	if (wide) { const cfhd_u2 v = CFHD_LDG64(p); w[0] = v.x; w[1] = v.y; }
	else { w[0] = CFHD_LDG32(p); w[1] = CFHD_LDG32(p + 4); }
}

__global__ void __launch_bounds__(DEC_THUMB_THREADS) k_dec_thumbnail(const DecLowpassJob *jobs, int nch, const uint32_t *verdicts, const uint32_t *marks, int width, int height, int yuv422,
                                                                     uint8_t *pictures, size_t picture_bytes)
{
	const int i = (int)blockIdx.y;
	const int pixels = width * height;
	const int first = (int)(blockIdx.x * DEC_THUMB_THREADS + threadIdx.x), step = (int)(gridDim.x * DEC_THUMB_THREADS);
	uint8_t *pic = pictures + picture_bytes * (size_t)i;
	const DecLowpassJob j0 = jobs[(size_t)i * nch], j1 = jobs[(size_t)i * nch + 1], j2 = jobs[(size_t)i * nch + 2];
	const int cw = yuv422 ? width / 2 : width;
	const bool clean = (verdicts[i] & 0xffu) == 0u && !marks[i] && j0.src && j1.src && j2.src && j0.width == width && j1.width == cw && j2.width == cw &&
	                   j0.height == height && j1.height == height && j2.height == height;
	if (!clean) {                                                // (the same for every lane of the workgroup)
		for (int p = 2 * first; p < pixels; p += 2 * step) store_u32x2_dword_aligned((uint32_t *)(pic + 4 * (size_t)p), 0u, 0u);
		return;
	}
	const int groups = pixels / DEC_THUMB_PIXELS;
	const bool wide_out = !((uintptr_t)pic & 15);
	const bool wide0 = !((uintptr_t)j0.src & 15), wide1 = !((uintptr_t)j1.src & (yuv422 ? 7 : 15)), wide2 = !((uintptr_t)j2.src & (yuv422 ? 7 : 15));
	for (int g = first; g < groups; g += step) {
		uint32_t a[4], o[8];
		thumb_load16(j0.src + 16 * (size_t)g, wide0, a);
		if (yuv422) {
			uint32_t c1[2], c2[2];
			thumb_load8(j1.src + 8 * (size_t)g, wide1, c1);
			thumb_load8(j2.src + 8 * (size_t)g, wide2, c2);
			for (int k = 0; k < 4; k++) {                        // pixel pair k: a longword of luma, a word of each chroma channel
				const int cr = ((k & 1) ? thumb_second10(c1[k >> 1]) : thumb_first10(c1[k >> 1])) - 512;
				const int cb = ((k & 1) ? thumb_second10(c2[k >> 1]) : thumb_first10(c2[k >> 1])) - 512;
				o[2 * k] = thumb_yuv(thumb_first10(a[k]) - 64, cr, cb);
				o[2 * k + 1] = thumb_yuv(thumb_second10(a[k]) - 64, cr, cb);
			}
		} else {
			uint32_t c1[4], c2[4];
			thumb_load16(j1.src + 16 * (size_t)g, wide1, c1);
			thumb_load16(j2.src + 16 * (size_t)g, wide2, c2);
			for (int k = 0; k < 4; k++) {
				o[2 * k] = thumb_dpx0(thumb_first10(c1[k]), thumb_first10(a[k]), thumb_first10(c2[k]));
				o[2 * k + 1] = thumb_dpx0(thumb_second10(c1[k]), thumb_second10(a[k]), thumb_second10(c2[k]));
			}
		}
		uint8_t *at = pic + 32 * (size_t)g;
		if (wide_out) { store_u32x4_global(at, o[0], o[1], o[2], o[3]); store_u32x4_global(at + 16, o[4], o[5], o[6], o[7]); }
		else for (int k = 0; k < 4; k++) store_u32x2_dword_aligned((uint32_t *)(at + 8 * k), o[2 * k], o[2 * k + 1]);
	}
	// the pairs behind the last whole group: up to three, a lane of the last piece each
	const int p = DEC_THUMB_PIXELS * groups + 2 * (int)threadIdx.x;
	if (blockIdx.x == gridDim.x - 1 && p < pixels) {
		const uint32_t l = CFHD_LDG32(j0.src + 2 * (size_t)p);
		uint32_t o0, o1;
		if (yuv422) {
			const int cr = thumb_first10(*(const uint16_t *)(j1.src + p)) - 512, cb = thumb_first10(*(const uint16_t *)(j2.src + p)) - 512;
			o0 = thumb_yuv(thumb_first10(l) - 64, cr, cb); o1 = thumb_yuv(thumb_second10(l) - 64, cr, cb);
		} else {
			const uint32_t l1 = CFHD_LDG32(j1.src + 2 * (size_t)p), l2 = CFHD_LDG32(j2.src + 2 * (size_t)p);
			o0 = thumb_dpx0(thumb_first10(l1), thumb_first10(l), thumb_first10(l2)); o1 = thumb_dpx0(thumb_second10(l1), thumb_second10(l), thumb_second10(l2));
		}
		store_u32x2_dword_aligned((uint32_t *)(pic + 4 * (size_t)p), o0, o1);
	}
}

} // namespace dev
} // namespace cfhd
