// cfhd_collect_kernels.h -- k_enc_collect, the mirror image of k_dec_deliver (cfhd_deliver_kernels.h) on the frame queue's side: a run of frames that lie in the caller's
// device memory as planar R, G, B tensors of u16, f16 or f32 elements (a torch tensor N x 3 x H x W) into the batch's RG48 frame slots, one launch for the whole run
// (cfhd_amd_batch_upload_device_planar, cfhd_device.hip collect_planar_frames) -- and k_enc_collect_bayer, the same for the BYR4 frames of a Bayer batch out of four
// planes, one per position of the 2 x 2 quad (N x 4 x H/2 x W/2).
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

} // namespace dev
} // namespace cfhd
