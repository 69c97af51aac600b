// cfhd_collect_kernels.h -- k_enc_collect, the mirror image of k_dec_deliver (cfhd_deliver_kernels.h) on the frame queue's side: a run of frames that lie in the caller's
// device memory as planar R, G, B tensors of u16, f16 or f32 elements (a torch tensor N x 3 x H x W) into the batch's RG48 frame slots, one launch for the whole run
// (cfhd_amd_batch_upload_device_planar, cfhd_device.hip collect_planar_frames) -- and k_enc_collect_bayer, the same for the BYR4 frames of a Bayer batch out of four
// planes, one per position of the 2 x 2 quad (N x 4 x H/2 x W/2), and k_enc_collect_yuv422, the same for the packed 4:2:2 frames (YUY2, 2vuy, YU64) of a batch out of
// a luma plane and two chroma planes of half the width (I422), and k_enc_collect_rgba, the same for the four-component frames (b64a, BGRA, BGRa) of a batch out of
// four planes R, G, B, A, top row first (N x 4 x H x W).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <cfhd_gfx950.h>

namespace cfhd {
namespace dev {

// (the values of CFHD_AMD_FRAMES_PLANAR_* in include/cfhd_amd.h, which are those of CFHD_AMD_PICTURES_PLANAR_*)
enum { COLLECT_PLANAR_U16 = 1, COLLECT_PLANAR_F16 = 2, COLLECT_PLANAR_F32 = 3, COLLECT_BAYER_U16 = 4, COLLECT_BAYER_F16 = 5, COLLECT_BAYER_F32 = 6 };
inline bool collect_is_bayer(int layout) { return layout >= COLLECT_BAYER_U16 && layout <= COLLECT_BAYER_F32; }
// the element type of a BAYER_* layout as the PLANAR_* value the element rules below are written for
inline int collect_bayer_element(int layout) { return layout - COLLECT_BAYER_U16 + COLLECT_PLANAR_U16; }
// (CFHD_AMD_FRAMES_YUV422_*) and the packed orders they are collected into: Y0 U Y1 V bytes, U Y0 V Y1 bytes, Y0 Cr Y1 Cb words
enum { COLLECT_YUV422_U8 = 7, COLLECT_YUV422_U16 = 8, COLLECT_YUV422_F16 = 9, COLLECT_YUV422_F32 = 10 };
enum { COLLECT_ORDER_YUY2 = 0, COLLECT_ORDER_2VUY = 1, COLLECT_ORDER_YU64 = 2 };
inline bool collect_is_yuv422(int layout) { return layout >= COLLECT_YUV422_U8 && layout <= COLLECT_YUV422_F32; }
inline int collect_yuv422_element_bytes(int layout) { return layout == COLLECT_YUV422_U8 ? 1 : (layout == COLLECT_YUV422_F32 ? 4 : 2); }

// The element rules, element -> RG48 word w.  U16: w is the element.  F32: t = x * 65535.0f, one IEEE single multiply; NaN gives 0; t clamped to [0, 65535] and
// rounded to nearest, ties to even (-0, everything negative, -inf: 0; everything >= 1, +inf: 65535).  F16: the binary16 value widened exactly to single, subnormals
// kept, then the F32 rule.  These invert the delivery rules where that is possible: collect(deliver(w)) = w for all 65 536 words through U16 and F32 (the three
// roundings of w / 65535 * 65535 stay within 0.012 of a word), and delivering a collected F16 tensor as F16 again returns the bit pattern of every element that F16
// delivery can produce.  Under device compilation the widening is the hardware's convert (v_cvt_f32_f16) and the rounding v_rndne_f32, in the default modes (round to
// nearest even, denormals kept); on a host-compiled build the widening is integer arithmetic on the bits.
__host__ __device__ inline float collect_f16_value(uint32_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
#else
	const uint32_t sign = (h & 0x8000u) << 16;
	uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu, x;
	if (e == 0x1fu) x = sign | 0x7f800000u | (m << 13);                         // infinity, NaN
	else if (e) x = sign | ((e + 112u) << 23) | (m << 13);                      // a normal binary16
	else if (m) {                                                               // a subnormal one, m * 2^-24: a normal single
		e = 113u;
		while (!(m & 0x400u)) { m <<= 1; e--; }
		x = sign | (e << 23) | ((m & 0x3ffu) << 13);
	} else x = sign;
	float f; memcpy(&f, &x, 4);
	return f;
#endif
}
__host__ __device__ inline uint32_t collect_word_f32(float x)
{
	float t = x * 65535.0f;
	t = t > 0.0f ? t : 0.0f;                   // (NaN compares false: 0; so do -0 and everything negative)
	t = t < 65535.0f ? t : 65535.0f;
	return (uint32_t)__builtin_rintf(t);       // to nearest, ties to even (the default rounding mode)
}
__host__ __device__ inline uint32_t collect_word_f16(uint32_t h) { return collect_word_f32(collect_f16_value(h)); }
// ... and the same rules with the unit of the word: 255 for the bytes of YUY2 and 2vuy, 65535 for the words of YU64 (the 4:2:2 plane layouts).  For the 8-bit unit
// collect(deliver(b)) = b for all 256 bytes through U8, F32 and F16 alike: the binary16 values of b / 255 are 256 distinct numbers that come back within 0.063 of b.
template <int UNIT> __host__ __device__ inline uint32_t collect_word_f32_of(float x)
{
	float t = x * (float)UNIT;
	t = t > 0.0f ? t : 0.0f;
	t = t < (float)UNIT ? t : (float)UNIT;
	return (uint32_t)__builtin_rintf(t);
}
template <int UNIT> __host__ __device__ inline uint32_t collect_word_f16_of(uint32_t h) { return collect_word_f32_of<UNIT>(collect_f16_value(h)); }

// two 16-bit words of two longwords into one: (a.lo, b.lo), (a.lo, b.hi), (a.hi, b.hi) as (low word, high word)
__device__ __forceinline__ uint32_t collect_lo_lo(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x05040100u); }
__device__ __forceinline__ uint32_t collect_lo_hi(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x07060100u); }
__device__ __forceinline__ uint32_t collect_hi_hi(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x07060302u); }

// eight elements of one plane (at, a multiple of 16: 16 bytes of u16 or f16, 32 bytes of f32) as RG48 words, two to a longword in element order
__device__ __forceinline__ void collect_load_plane(const uint8_t *at, int layout, uint32_t p[4])
{
	const cfhd_u4 v = CFHD_LDG128(at);
	if (layout == COLLECT_PLANAR_U16) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; return; }
	if (layout == COLLECT_PLANAR_F16) {
		const uint32_t h[4] = { v.x, v.y, v.z, v.w };
		for (int k = 0; k < 4; k++) p[k] = collect_word_f16(h[k] & 0xffffu) | (collect_word_f16(h[k] >> 16) << 16);
		return;
	}
	const cfhd_u4 u = CFHD_LDG128(at + 16);
	const uint32_t bits[8] = { v.x, v.y, v.z, v.w, u.x, u.y, u.z, u.w };
	for (int k = 0; k < 4; k++) {
		float lo, hi; memcpy(&lo, &bits[2 * k], 4); memcpy(&hi, &bits[2 * k + 1], 4);
		p[k] = collect_word_f32(lo) | (collect_word_f32(hi) << 16);
	}
}

// ---------------------------------------------------------------------------------------------
// k_enc_collect: frame i of the run out of src + i * src_stride -- three planes R, G, B, each `rows` rows of `width` elements, rows src_pitch bytes apart, planes
// rows * src_pitch apart -- into dst + i * dst_stride, the batch's own RG48 frames: `rows` rows of 6 x width bytes back to back.  The source is read, never written.
//   A lane takes 8 pixels: one 16-byte load per plane for u16 / f16, two for f32 -- the loads of a wave cover consecutive bytes of a plane row --, the elements turned
//   into words in registers, the 24 words interleaved (v_perm: R0 G0 | B0 R1 | G1 B1 of every pair of pixels), three 16-byte stores of 48 consecutive bytes: a wave
//   writes 3 KB of the frame row without a gap.
//   Every RG48 batch has a width that is a multiple of 8 (build_frame_plan in cfhd_tables.cpp and build_gop_plan in cfhd_gop.cpp admit no other), its frame slots come from
//   hipMalloc and lie 6 x width x rows apart, and the entry point admits only pointers, strides and pitches that are multiples of 16: every row on either side starts
//   on a 16-byte boundary and is a whole number of groups of eight.  There is no element-by-element path.
// No LDS, no scratch.  A wave owns a row at a time: grid (row pieces, frames), ENC_COLLECT_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
enum { ENC_COLLECT_THREADS = 256, ENC_COLLECT_WAVES = ENC_COLLECT_THREADS / 64, ENC_COLLECT_SPLIT = 32 };
inline unsigned enc_collect_pieces(int rows) { const int p = (rows + ENC_COLLECT_WAVES - 1) / ENC_COLLECT_WAVES; return (unsigned)(p < 1 ? 1 : (p > ENC_COLLECT_SPLIT ? ENC_COLLECT_SPLIT : p)); }

__global__ void __launch_bounds__(ENC_COLLECT_THREADS) k_enc_collect(const uint8_t *src, size_t src_stride, int src_pitch, int rows, int width, uint8_t *dst, size_t dst_stride, int layout)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *in = src + src_stride * (size_t)blockIdx.y;
	uint8_t *frame = dst + dst_stride * (size_t)blockIdx.y;
	const int elt = layout == COLLECT_PLANAR_F32 ? 4 : 2, groups = width >> 3;
	const size_t plane = (size_t)src_pitch * (size_t)rows;
	for (int r = (int)blockIdx.x * ENC_COLLECT_WAVES + wave; r < rows; r += (int)gridDim.x * ENC_COLLECT_WAVES) {
		const uint8_t *irow = in + (size_t)r * src_pitch;
		uint8_t *orow = frame + (size_t)r * 6 * width;
		for (int g = lane; g < groups; g += 64) {
			const uint8_t *at = irow + (size_t)g * 8 * elt;
			uint32_t R[4], G[4], B[4];
			collect_load_plane(at, layout, R);
			collect_load_plane(at + plane, layout, G);
			collect_load_plane(at + 2 * plane, layout, B);
			uint32_t o[12];
			for (int k = 0; k < 4; k++) { o[3 * k] = collect_lo_lo(R[k], G[k]); o[3 * k + 1] = collect_lo_hi(B[k], R[k]); o[3 * k + 2] = collect_hi_hi(G[k], B[k]); }
			uint8_t *to = orow + 48 * g;
			store_u32x4_global(to, o[0], o[1], o[2], o[3]);
			store_u32x4_global(to + 16, o[4], o[5], o[6], o[7]);
			store_u32x4_global(to + 32, o[8], o[9], o[10], o[11]);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// k_enc_collect_bayer: the mirror image of k_dec_deliver_bayer.  Frame i of the run out of src + i * src_stride -- four planes, one per position of the 2 x 2 quad
// (plane k = 2 * (row & 1) + (column & 1); red-green phase: R, G1, G2, B), each quad_rows rows of `width` elements, rows src_pitch bytes apart, planes quad_rows *
// src_pitch apart -- into dst + i * dst_stride, the batch's own BYR4 frames: 2 x quad_rows mosaic rows of 4 x width bytes back to back.  The source is read, never
// written.  `layout`: the element type as COLLECT_PLANAR_U16 / _F16 / _F32 (collect_bayer_element), the element rules those of collect_load_plane.
//   A wave owns a quad row at a time.  A lane takes 8 quads: one collect_load_plane per plane (a 16-byte load for u16 / f16, two for f32; the loads of a wave cover
//   consecutive bytes of a plane row), planes 0 and 1 interleaved into the even mosaic row, 2 and 3 into the odd one (v_perm_b32: 8 per mosaic row), two 16-byte stores
//   of 32 consecutive bytes into each: a wave writes 2 KB of each mosaic row without a gap.
//   Every BYR4 batch has component planes of whole groups of eight (build_frame_plan), its frame slots come from hipMalloc and lie 8 x width x quad_rows apart, and
//   the entry point admits only pointers, strides and pitches that are multiples of 16 (collect_planar_frames checks all of it): no element-by-element path.
// No LDS, no scratch.  Grid (pieces of quad rows: enc_collect_pieces(quad_rows), frames), ENC_COLLECT_WAVES quad rows per piece and step.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ENC_COLLECT_THREADS) k_enc_collect_bayer(const uint8_t *src, size_t src_stride, int src_pitch, int quad_rows, int width, uint8_t *dst, size_t dst_stride, int layout)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *in = src + src_stride * (size_t)blockIdx.y;
	uint8_t *frame = dst + dst_stride * (size_t)blockIdx.y;
	const int elt = layout == COLLECT_PLANAR_F32 ? 4 : 2, groups = width >> 3;
	const size_t plane = (size_t)src_pitch * (size_t)quad_rows;
	for (int q = (int)blockIdx.x * ENC_COLLECT_WAVES + wave; q < quad_rows; q += (int)gridDim.x * ENC_COLLECT_WAVES) {
		const uint8_t *irow = in + (size_t)q * src_pitch;
		uint8_t *even = frame + (size_t)q * 8 * width, *odd = even + (size_t)4 * width;
		for (int g = lane; g < groups; g += 64) {
			const uint8_t *at = irow + (size_t)g * 8 * elt;
			uint32_t A[4], B[4], C[4], D[4];
			collect_load_plane(at, layout, A);
			collect_load_plane(at + plane, layout, B);
			collect_load_plane(at + 2 * plane, layout, C);
			collect_load_plane(at + 3 * plane, layout, D);
			uint32_t e[8], o[8];
			for (int k = 0; k < 4; k++) { e[2 * k] = collect_lo_lo(A[k], B[k]); e[2 * k + 1] = collect_hi_hi(A[k], B[k]); o[2 * k] = collect_lo_lo(C[k], D[k]); o[2 * k + 1] = collect_hi_hi(C[k], D[k]); }
			store_u32x4_global(even + 32 * g, e[0], e[1], e[2], e[3]);
			store_u32x4_global(even + 32 * g + 16, e[4], e[5], e[6], e[7]);
			store_u32x4_global(odd + 32 * g, o[0], o[1], o[2], o[3]);
			store_u32x4_global(odd + 32 * g + 16, o[4], o[5], o[6], o[7]);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// k_enc_collect_yuv422: the mirror image of k_dec_deliver_yuv422.  Frame i of the run out of src + i * src_stride -- three planes in the I422 convention: Y, `rows` rows
// of `width` elements src_pitch bytes apart, at 0; Cb, `rows` rows of width / 2 elements src_pitch / 2 bytes apart, at rows * src_pitch; Cr, the same, behind it -- into
// dst + i * dst_stride, the batch's own packed 4:2:2 frames: `rows` rows back to back, 2 x width bytes a row (order COLLECT_ORDER_YUY2: Y0 U Y1 V, _2VUY: U Y0 V Y1)
// or 4 x width (_YU64: the words Y0 Cr Y1 Cb).  The source is read, never written.  `layout`: COLLECT_YUV422_U8 (8-bit frames) / _U16 (YU64) -- the element as it is --,
// _F16 / _F32: collect_word_f32_of with the unit of the frame's own word, 255 or 65535.
//   A wave owns a row at a time, a lane takes 16 pixels: 16 elements of the luma row and 8 of each chroma row -- 16-byte loads, one 8-byte load per chroma plane for
//   U8; the loads of a wave cover consecutive bytes of a plane row --, the elements turned into bytes or words in registers and interleaved (v_perm_b32: 12 for the
//   8-bit orders, 16 for YU64), then two (8-bit) or four (YU64) 16-byte stores of 32 or 64 consecutive bytes: a wave writes 2 or 4 KB of the frame row without a gap.
//   Every 4:2:2 plan has a width that is a multiple of 16 (build_frame_plan in cfhd_tables.cpp: chroma planes of whole groups of eight; build_gop_plan in cfhd_gop.cpp),
//   the frame slots come from hipMalloc and lie rows x row bytes apart, and the entry point admits only pointers and strides that are multiples of 16 and pitches that
//   are multiples of 32 (collect_planar_frames checks all of it): every row on either side starts on a 16-byte boundary and is a whole number of groups.  There is
//   no tail path.
// No LDS, no scratch.  Grid (row pieces: enc_collect_pieces(rows), frames), ENC_COLLECT_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
enum { ENC_COLLECT_YUV422_PIXELS = 16 };
__device__ __forceinline__ uint32_t collect_hi_lo(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x05040302u); }      // (a.hi, b.lo)

// B bytes (8 or a multiple of 16) at `at` as longwords
template <int B> __device__ __forceinline__ void collect_load_longwords(const uint8_t *at, uint32_t *d)
{
	if constexpr (B == 8) { const cfhd_u2 v = CFHD_LDG64(at); d[0] = v.x; d[1] = v.y; }
	else for (int k = 0; k < B / 16; k++) { const cfhd_u4 v = CFHD_LDG128(at + 16 * k); d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w; }
}
// N elements of one plane row as the frame's own bytes (UNIT 255: four to a longword) or words (UNIT 65535: two to a longword), in element order
template <int LAYOUT, int UNIT, int N> __device__ __forceinline__ void collect_load_elements(const uint8_t *at, uint32_t *out)
{
	constexpr int E = LAYOUT == COLLECT_YUV422_U8 ? 1 : (LAYOUT == COLLECT_YUV422_F32 ? 4 : 2);
	uint32_t d[N * E / 4];
	collect_load_longwords<N * E>(at, d);
	if constexpr (LAYOUT == COLLECT_YUV422_U8 || LAYOUT == COLLECT_YUV422_U16) { for (int k = 0; k < N * E / 4; k++) out[k] = d[k]; }
	else {
		uint32_t w[N];
		for (int k = 0; k < N; k++) {
			if constexpr (LAYOUT == COLLECT_YUV422_F32) { float x; memcpy(&x, &d[k], 4); w[k] = collect_word_f32_of<UNIT>(x); }
			else w[k] = collect_word_f16_of<UNIT>((d[k / 2] >> (16 * (k & 1))) & 0xffffu);
		}
		if constexpr (UNIT == 255) { for (int k = 0; k < N / 4; k++) out[k] = w[4 * k] | (w[4 * k + 1] << 8) | (w[4 * k + 2] << 16) | (w[4 * k + 3] << 24); }
		else for (int k = 0; k < N / 2; k++) out[k] = w[2 * k] | (w[2 * k + 1] << 16);
	}
}
// one row of `width` pixels
template <int ORDER, int LAYOUT> __device__ __forceinline__ void collect_yuv422_row(const uint8_t *y, const uint8_t *cb, const uint8_t *cr, int width, uint8_t *orow, int lane)
{
	constexpr int E = LAYOUT == COLLECT_YUV422_U8 ? 1 : (LAYOUT == COLLECT_YUV422_F32 ? 4 : 2), P = ENC_COLLECT_YUV422_PIXELS;
	const int groups = width / P;
	for (int g = lane; g < groups; g += 64) {
		if constexpr (ORDER == COLLECT_ORDER_YU64) {
			uint32_t Y[P / 2], U[P / 4], V[P / 4], o[P];
			collect_load_elements<LAYOUT, 65535, P>(y + (size_t)g * P * E, Y);
			collect_load_elements<LAYOUT, 65535, P / 2>(cb + (size_t)g * (P / 2) * E, U);
			collect_load_elements<LAYOUT, 65535, P / 2>(cr + (size_t)g * (P / 2) * E, V);
			// the longwords (Y0, Cr), (Y1, Cb) of every pair of pixels; a chroma longword serves two pairs
			for (int m = 0; m < P / 4; m++) {
				o[4 * m] = collect_lo_lo(Y[2 * m], V[m]); o[4 * m + 1] = collect_hi_lo(Y[2 * m], U[m]);
				o[4 * m + 2] = collect_lo_hi(Y[2 * m + 1], V[m]); o[4 * m + 3] = collect_hi_hi(Y[2 * m + 1], U[m]);
			}
			uint8_t *to = orow + (size_t)g * 4 * P;
			for (int k = 0; k < P; k += 4) store_u32x4_global(to + 4 * k, o[k], o[k + 1], o[k + 2], o[k + 3]);
		} else {
			uint32_t Y[P / 4], U[P / 8], V[P / 8], o[P / 2];
			collect_load_elements<LAYOUT, 255, P>(y + (size_t)g * P * E, Y);
			collect_load_elements<LAYOUT, 255, P / 2>(cb + (size_t)g * (P / 2) * E, U);
			collect_load_elements<LAYOUT, 255, P / 2>(cr + (size_t)g * (P / 2) * E, V);
			// a longword per pair of pixels: two luma bytes (selector bytes 0 .. 3) and the pair's Cb Cr out of the interleaved chroma (4 .. 7)
			constexpr uint32_t even = ORDER == COLLECT_ORDER_YUY2 ? 0x05010400u : 0x01050004u, odd = ORDER == COLLECT_ORDER_YUY2 ? 0x07030602u : 0x03070206u;
			for (int m = 0; m < P / 8; m++) {
				const uint32_t uv0 = byte_perm(V[m], U[m], 0x05010400u), uv1 = byte_perm(V[m], U[m], 0x07030602u);      // Cb0 Cr0 Cb1 Cr1, Cb2 Cr2 Cb3 Cr3
				o[4 * m] = byte_perm(uv0, Y[2 * m], even); o[4 * m + 1] = byte_perm(uv0, Y[2 * m], odd);
				o[4 * m + 2] = byte_perm(uv1, Y[2 * m + 1], even); o[4 * m + 3] = byte_perm(uv1, Y[2 * m + 1], odd);
			}
			uint8_t *to = orow + (size_t)g * 2 * P;
			for (int k = 0; k < P / 2; k += 4) store_u32x4_global(to + 4 * k, o[k], o[k + 1], o[k + 2], o[k + 3]);
		}
	}
}

__global__ void __launch_bounds__(ENC_COLLECT_THREADS) k_enc_collect_yuv422(const uint8_t *src, size_t src_stride, int src_pitch, int rows, int width, uint8_t *dst, size_t dst_stride, int layout, int order)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *in = src + src_stride * (size_t)blockIdx.y;
	uint8_t *frame = dst + dst_stride * (size_t)blockIdx.y;
	const int row_bytes = (order == COLLECT_ORDER_YU64 ? 4 : 2) * width, chroma_pitch = src_pitch >> 1;
	const uint8_t *cb_plane = in + (size_t)src_pitch * (size_t)rows, *cr_plane = cb_plane + (size_t)chroma_pitch * (size_t)rows;
	for (int r = (int)blockIdx.x * ENC_COLLECT_WAVES + wave; r < rows; r += (int)gridDim.x * ENC_COLLECT_WAVES) {
		const uint8_t *y = in + (size_t)r * src_pitch, *cb = cb_plane + (size_t)r * chroma_pitch, *cr = cr_plane + (size_t)r * chroma_pitch;
		uint8_t *orow = frame + (size_t)r * row_bytes;
		if (order == COLLECT_ORDER_YU64) {
			if (layout == COLLECT_YUV422_U16) collect_yuv422_row<COLLECT_ORDER_YU64, COLLECT_YUV422_U16>(y, cb, cr, width, orow, lane);
			else if (layout == COLLECT_YUV422_F16) collect_yuv422_row<COLLECT_ORDER_YU64, COLLECT_YUV422_F16>(y, cb, cr, width, orow, lane);
			else collect_yuv422_row<COLLECT_ORDER_YU64, COLLECT_YUV422_F32>(y, cb, cr, width, orow, lane);
		} else if (order == COLLECT_ORDER_YUY2) {
			if (layout == COLLECT_YUV422_U8) collect_yuv422_row<COLLECT_ORDER_YUY2, COLLECT_YUV422_U8>(y, cb, cr, width, orow, lane);
			else if (layout == COLLECT_YUV422_F16) collect_yuv422_row<COLLECT_ORDER_YUY2, COLLECT_YUV422_F16>(y, cb, cr, width, orow, lane);
			else collect_yuv422_row<COLLECT_ORDER_YUY2, COLLECT_YUV422_F32>(y, cb, cr, width, orow, lane);
		} else {
			if (layout == COLLECT_YUV422_U8) collect_yuv422_row<COLLECT_ORDER_2VUY, COLLECT_YUV422_U8>(y, cb, cr, width, orow, lane);
			else if (layout == COLLECT_YUV422_F16) collect_yuv422_row<COLLECT_ORDER_2VUY, COLLECT_YUV422_F16>(y, cb, cr, width, orow, lane);
			else collect_yuv422_row<COLLECT_ORDER_2VUY, COLLECT_YUV422_F32>(y, cb, cr, width, orow, lane);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// k_enc_collect_rgba: the mirror image of k_dec_deliver_rgba.  Frame i of the run out of src + i * src_stride -- four planes R, G, B, A, top row first, each `rows` rows
// of `width` elements, rows src_pitch bytes apart, planes rows * src_pitch apart -- into dst + i * dst_stride, the batch's own packed frames: `rows` rows back to back,
// 8 x width bytes a row (order COLLECT_ORDER_B64A: the native 16-bit words A R G B) or 4 x width (_BGRA, _BGRa: the bytes B G R A).  A BGRA frame lies bottom row first
// in its slot: plane row r goes to slot row rows - 1 - r, an address.  The source is read, never written.  `layout`: COLLECT_RGBA_U8 (BGRA / BGRa) / _U16 (b64a) -- the
// element as it is --, _F16 / _F32: collect_word_f32_of with the unit of the frame's own word, 255 or 65535.  Alpha is a component like the others.
//   A wave owns a row at a time.  b64a: a lane takes 8 pixels, 8 elements of each plane row (one 16-byte load per plane for u16 / f16, two for f32), the words of two
//   pixels per plane longword dealt to the longwords (A, R), (G, B) of each pixel (v_perm_b32: 16), four 16-byte stores of 64 consecutive bytes: a wave writes 4 KB of
//   the frame row without a gap.  BGRA / BGRa: 16 pixels for U8 and F16 (one or two 16-byte loads per plane), 8 for F32 (two); the bytes of four pixels per plane
//   longword transposed in two rounds of v_perm_b32 (8 per four pixels), four or two 16-byte stores of consecutive bytes.  The loads of a wave cover consecutive bytes
//   of a plane row.
//   The columns behind the last whole group go element by element (no plan of these formats is known to have any: build_frame_plan, build_gop_plan).  The frame slots
//   come from hipMalloc and lie rows x row bytes apart, the entry point admits only slot rows, pointers, strides and pitches that are multiples of 16
//   (collect_planar_frames checks all of it): every row on either side starts on a 16-byte boundary.
// No LDS, no scratch.  Grid (row pieces: enc_collect_pieces(rows), frames), ENC_COLLECT_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
// (CFHD_AMD_FRAMES_RGBA_*) and the packed orders they are collected into
enum { COLLECT_RGBA_U8 = 11, COLLECT_RGBA_U16 = 12, COLLECT_RGBA_F16 = 13, COLLECT_RGBA_F32 = 14 };
enum { COLLECT_ORDER_B64A = 0, COLLECT_ORDER_BGRA = 1, COLLECT_ORDER_BGRa = 2 };
inline bool collect_is_rgba(int layout) { return layout >= COLLECT_RGBA_U8 && layout <= COLLECT_RGBA_F32; }
inline int collect_rgba_element_bytes(int layout) { return layout == COLLECT_RGBA_U8 ? 1 : (layout == COLLECT_RGBA_F32 ? 4 : 2); }
// the element type of an RGBA_* layout as the YUV422_* value collect_load_elements is written for
template <int LAYOUT> struct collect_rgba_as_yuv422 { static constexpr int value = LAYOUT - COLLECT_RGBA_U8 + COLLECT_YUV422_U8; };

// one element of a plane row as the frame's own byte or word (the columns behind the last whole group)
template <int LAYOUT, int UNIT> __device__ __forceinline__ uint32_t collect_rgba_element(const uint8_t *plane_row, int x)
{
	if constexpr (LAYOUT == COLLECT_RGBA_U8) return plane_row[x];
	else if constexpr (LAYOUT == COLLECT_RGBA_U16) return ((const uint16_t *)plane_row)[x];
	else if constexpr (LAYOUT == COLLECT_RGBA_F16) return collect_word_f16_of<UNIT>(((const uint16_t *)plane_row)[x]);
	else return collect_word_f32_of<UNIT>(((const float *)plane_row)[x]);
}
// one row of `width` pixels out of row `irow` of plane R (the planes `plane` bytes apart) into a b64a frame row
template <int LAYOUT> __device__ __forceinline__ void collect_rgba_row_words(const uint8_t *irow, size_t plane, int width, uint8_t *orow, int lane)
{
	constexpr int E = LAYOUT == COLLECT_RGBA_F32 ? 4 : 2, L = collect_rgba_as_yuv422<LAYOUT>::value;
	const int groups = width >> 3;
	for (int g = lane; g < groups; g += 64) {
		const uint8_t *at = irow + (size_t)g * 8 * E;
		uint32_t R[4], G[4], B[4], A[4], o[16];
		collect_load_elements<L, 65535, 8>(at, R);
		collect_load_elements<L, 65535, 8>(at + plane, G);
		collect_load_elements<L, 65535, 8>(at + 2 * plane, B);
		collect_load_elements<L, 65535, 8>(at + 3 * plane, A);
		for (int k = 0; k < 4; k++) {
			o[4 * k] = collect_lo_lo(A[k], R[k]); o[4 * k + 1] = collect_lo_lo(G[k], B[k]);
			o[4 * k + 2] = collect_hi_hi(A[k], R[k]); o[4 * k + 3] = collect_hi_hi(G[k], B[k]);
		}
		uint8_t *to = orow + 64 * (size_t)g;
		for (int k = 0; k < 16; k += 4) store_u32x4_global(to + 4 * k, o[k], o[k + 1], o[k + 2], o[k + 3]);
	}
	for (int x = 8 * groups + lane; x < width; x += 64) {
		const uint32_t r = collect_rgba_element<LAYOUT, 65535>(irow, x), g = collect_rgba_element<LAYOUT, 65535>(irow + plane, x);
		const uint32_t b = collect_rgba_element<LAYOUT, 65535>(irow + 2 * plane, x), a = collect_rgba_element<LAYOUT, 65535>(irow + 3 * plane, x);
		uint32_t *to = (uint32_t *)(orow + 8 * (size_t)x);
		to[0] = a | (r << 16); to[1] = g | (b << 16);
	}
}
// ... into a row of B G R A bytes
template <int LAYOUT> __device__ __forceinline__ void collect_rgba_row_bytes(const uint8_t *irow, size_t plane, int width, uint8_t *orow, int lane)
{
	constexpr int E = LAYOUT == COLLECT_RGBA_U8 ? 1 : (LAYOUT == COLLECT_RGBA_F32 ? 4 : 2), P = LAYOUT == COLLECT_RGBA_F32 ? 8 : 16, L = collect_rgba_as_yuv422<LAYOUT>::value;
	const int groups = width / P;
	for (int g = lane; g < groups; g += 64) {
		const uint8_t *at = irow + (size_t)g * P * E;
		uint32_t R[P / 4], G[P / 4], B[P / 4], A[P / 4], o[P];
		collect_load_elements<L, 255, P>(at, R);
		collect_load_elements<L, 255, P>(at + plane, G);
		collect_load_elements<L, 255, P>(at + 2 * plane, B);
		collect_load_elements<L, 255, P>(at + 3 * plane, A);
		for (int m = 0; m < P / 4; m++) {
			// B0 G0 B1 G1 | B2 G2 B3 G3 and R0 A0 R1 A1 | R2 A2 R3 A3, then a longword per pixel
			const uint32_t bg01 = byte_perm(G[m], B[m], 0x05010400u), bg23 = byte_perm(G[m], B[m], 0x07030602u);
			const uint32_t ra01 = byte_perm(A[m], R[m], 0x05010400u), ra23 = byte_perm(A[m], R[m], 0x07030602u);
			o[4 * m] = collect_lo_lo(bg01, ra01); o[4 * m + 1] = collect_hi_hi(bg01, ra01);
			o[4 * m + 2] = collect_lo_lo(bg23, ra23); o[4 * m + 3] = collect_hi_hi(bg23, ra23);
		}
		uint8_t *to = orow + 4 * P * (size_t)g;
		for (int k = 0; k < P; k += 4) store_u32x4_global(to + 4 * k, o[k], o[k + 1], o[k + 2], o[k + 3]);
	}
	for (int x = P * groups + lane; x < width; x += 64) {
		const uint32_t r = collect_rgba_element<LAYOUT, 255>(irow, x), g = collect_rgba_element<LAYOUT, 255>(irow + plane, x);
		const uint32_t b = collect_rgba_element<LAYOUT, 255>(irow + 2 * plane, x), a = collect_rgba_element<LAYOUT, 255>(irow + 3 * plane, x);
		*(uint32_t *)(orow + 4 * (size_t)x) = b | (g << 8) | (r << 16) | (a << 24);
	}
}

__global__ void __launch_bounds__(ENC_COLLECT_THREADS) k_enc_collect_rgba(const uint8_t *src, size_t src_stride, int src_pitch, int rows, int width, uint8_t *dst, size_t dst_stride, int layout, int order)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *in = src + src_stride * (size_t)blockIdx.y;
	uint8_t *frame = dst + dst_stride * (size_t)blockIdx.y;
	const int row_bytes = (order == COLLECT_ORDER_B64A ? 8 : 4) * width;
	const size_t plane = (size_t)src_pitch * (size_t)rows;
	for (int r = (int)blockIdx.x * ENC_COLLECT_WAVES + wave; r < rows; r += (int)gridDim.x * ENC_COLLECT_WAVES) {
		const uint8_t *irow = in + (size_t)r * src_pitch;
		uint8_t *orow = frame + (size_t)(order == COLLECT_ORDER_BGRA ? rows - 1 - r : r) * row_bytes;
		if (order == COLLECT_ORDER_B64A) {
			if (layout == COLLECT_RGBA_U16) collect_rgba_row_words<COLLECT_RGBA_U16>(irow, plane, width, orow, lane);
			else if (layout == COLLECT_RGBA_F16) collect_rgba_row_words<COLLECT_RGBA_F16>(irow, plane, width, orow, lane);
			else collect_rgba_row_words<COLLECT_RGBA_F32>(irow, plane, width, orow, lane);
		} else {
			if (layout == COLLECT_RGBA_U8) collect_rgba_row_bytes<COLLECT_RGBA_U8>(irow, plane, width, orow, lane);
			else if (layout == COLLECT_RGBA_F16) collect_rgba_row_bytes<COLLECT_RGBA_F16>(irow, plane, width, orow, lane);
			else collect_rgba_row_bytes<COLLECT_RGBA_F32>(irow, plane, width, orow, lane);
		}
	}
}

} // namespace dev
} // namespace cfhd
