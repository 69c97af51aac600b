// cfhd_deliver_kernels.h -- k_dec_deliver, the last kernel of a decode-queue pass that delivers into the caller's device memory (cfhd_amd_decode_batch_set_device_pictures,
// cfhd_decode_queue.hip): behind k_dec_blank, the pictures of the pass out of the batch's own tightly packed buffer into memory the caller owns -- as the packed
// pictures they are, at the caller's pitch, or, for RG48, as three planes R, G, B of u16, f16 or f32 elements (a torch tensor N x 3 x H x W) -- and k_dec_deliver_bayer,
// which takes its place for the BYR4 mosaics of a Bayer batch delivered as four planes, one per position of the 2 x 2 quad (N x 4 x H/2 x W/2), and k_dec_deliver_yuv422,
// which takes it for the packed 4:2:2 pictures (YUY2, 2vuy, YU64) delivered as a luma plane and two chroma planes of half the width (I422: N x [H x W | 2 x H x W/2]), and
// k_dec_deliver_rgba, which takes it for the four-component pictures (b64a, BGRA, BGRa) delivered as four planes R, G, B, A, top row first (N x 4 x H x W), and
// k_dec_deliver_rgb_as_yuv, which takes it for the RG48 pictures of RGB samples delivered as the YU64 picture the reference decodes such a sample to, packed or as
// Y, Cb, Cr planes, and k_dec_deliver_rgb10, which takes it for the DPX0 longwords of a thumbnail batch delivered as three planes R, G, B of their 10-bit values.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <cfhd_gfx950.h>

namespace cfhd {
namespace dev {

// (the values of CFHD_AMD_PICTURES_* in include/cfhd_amd.h)
enum { DELIVER_PACKED = 0, DELIVER_PLANAR_U16 = 1, DELIVER_PLANAR_F16 = 2, DELIVER_PLANAR_F32 = 3, DELIVER_BAYER_U16 = 4, DELIVER_BAYER_F16 = 5, DELIVER_BAYER_F32 = 6 };
inline bool deliver_is_bayer(int layout) { return layout >= DELIVER_BAYER_U16 && layout <= DELIVER_BAYER_F32; }
// the element type of a BAYER_* layout as the PLANAR_* value the element rules below are written for
inline int deliver_bayer_element(int layout) { return layout - DELIVER_BAYER_U16 + DELIVER_PLANAR_U16; }
// (CFHD_AMD_PICTURES_YUV422_*) and the packed orders they are written from: Y0 U Y1 V bytes, U Y0 V Y1 bytes, Y0 Cr Y1 Cb words
enum { DELIVER_YUV422_U8 = 7, DELIVER_YUV422_U16 = 8, DELIVER_YUV422_F16 = 9, DELIVER_YUV422_F32 = 10 };
enum { YUV422_YUY2 = 0, YUV422_2VUY = 1, YUV422_YU64 = 2 };
inline bool deliver_is_yuv422(int layout) { return layout >= DELIVER_YUV422_U8 && layout <= DELIVER_YUV422_F32; }
inline int deliver_yuv422_element_bytes(int layout) { return layout == DELIVER_YUV422_U8 ? 1 : (layout == DELIVER_YUV422_F32 ? 4 : 2); }

// The element rules of the planar layouts for the RG48 word w.  F32: (float)w * (1.0f / 65535.0f), one IEEE single multiply.  F16: that value rounded to nearest-even
// to binary16, subnormals kept (w = 1 .. 3 land there: 1 / 65535 < 2^-14) -- under device compilation the hardware's convert (v_cvt_pk_f16_f32 in the gfx950 build; the kernels run
// with the default mode: round to nearest even, 16-bit denormals kept), on a host-compiled build the same rule in integer arithmetic on the bits of the single.
__host__ __device__ inline float deliver_unit_f32(uint32_t w) { return (float)w * (1.0f / 65535.0f); }
// ... and the same rule with the unit of the word: 255 for the bytes of YUY2 and 2vuy, 65535 for the words of YU64 (the 4:2:2 plane layouts; F16 is deliver_f16_bits of it)
template <int UNIT> __host__ __device__ inline float deliver_unit_f32_of(uint32_t w) { return (float)w * (1.0f / (float)UNIT); }
__host__ __device__ inline uint32_t deliver_f16_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const _Float16 h = (_Float16)f;
	return (uint32_t)__builtin_bit_cast(unsigned short, h);
#else
	uint32_t x; memcpy(&x, &f, 4);
	const uint32_t sign = (x >> 16) & 0x8000u, e = (x >> 23) & 0xffu, m = x & 0x7fffffu;
	if (e == 0xffu) return sign | 0x7c00u | (m ? 0x200u | (m >> 13) : 0u);      // infinity, NaN (quiet)
	if (e >= 143u) return sign | 0x7c00u;                                        // 2^16 and beyond: infinity (65520 .. 65536 get there by the carry below)
	uint32_t h, rest, half;
	if (e >= 113u) { h = ((e - 112u) << 10) | (m >> 13); rest = m & 0x1fffu; half = 0x1000u; }      // a normal binary16: 13 bits of the fraction go
	else if (e >= 102u) { const uint32_t full = m | 0x800000u, shift = 126u - e; h = full >> shift; rest = full & ((1u << shift) - 1u); half = 1u << (shift - 1u); }      // a subnormal one: units of 2^-24
	else return sign;                                                            // below 2^-25 (zero, the singles' own subnormals): zero
	if (rest > half || (rest == half && (h & 1u))) h++;                          // to nearest, ties to even; a carry runs into the exponent, as it should
	return sign | h;
#endif
}

// the words (a.lo, b.hi) and (a.hi, b.lo) of two longwords
__device__ __forceinline__ uint32_t deliver_lo_hi(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x07060100u); }
__device__ __forceinline__ uint32_t deliver_hi_lo(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x05040302u); }
// ... and (a.lo, b.lo), (a.hi, b.hi): the even and the odd words of four
__device__ __forceinline__ uint32_t deliver_lo_lo(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x05040100u); }
__device__ __forceinline__ uint32_t deliver_hi_hi(uint32_t a, uint32_t b) { return byte_perm(b, a, 0x07060302u); }
__device__ __forceinline__ cfhd_u4 deliver_load_dword_aligned(const uint8_t *p) { cfhd_u4 v; v.x = CFHD_LDG32(p); v.y = CFHD_LDG32(p + 4); v.z = CFHD_LDG32(p + 8); v.w = CFHD_LDG32(p + 12); return v; }

// eight elements of one plane, two to a longword as they come out of the RG48 words: 16 bytes of u16 or f16, 32 bytes of f32 (at, a multiple of 16)
__device__ __forceinline__ void deliver_store_plane(uint8_t *at, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, int layout)
{
	if (layout == DELIVER_PLANAR_U16) { store_u32x4_global(at, p0, p1, p2, p3); return; }
	const uint32_t p[4] = { p0, p1, p2, p3 };
	if (layout == DELIVER_PLANAR_F16) {
		uint32_t h[4];
		for (int k = 0; k < 4; k++) h[k] = deliver_f16_bits(deliver_unit_f32(p[k] & 0xffffu)) | (deliver_f16_bits(deliver_unit_f32(p[k] >> 16)) << 16);
		store_u32x4_global(at, h[0], h[1], h[2], h[3]);
		return;
	}
	uint32_t f[8];
	for (int k = 0; k < 4; k++) { const float lo = deliver_unit_f32(p[k] & 0xffffu), hi = deliver_unit_f32(p[k] >> 16); memcpy(&f[2 * k], &lo, 4); memcpy(&f[2 * k + 1], &hi, 4); }
	store_u32x4_global(at, f[0], f[1], f[2], f[3]);
	store_u32x4_global(at + 16, f[4], f[5], f[6], f[7]);
}
// one element of a plane (the columns behind the last whole group of eight)
__device__ __forceinline__ void deliver_store_element(uint8_t *plane_row, int x, uint32_t w, int layout)
{
	if (layout == DELIVER_PLANAR_U16) ((uint16_t *)plane_row)[x] = (uint16_t)w;
	else if (layout == DELIVER_PLANAR_F16) ((uint16_t *)plane_row)[x] = (uint16_t)deliver_f16_bits(deliver_unit_f32(w));
	else ((float *)plane_row)[x] = deliver_unit_f32(w);
}

// ---------------------------------------------------------------------------------------------
// k_dec_deliver: picture i of the pass, `rows` rows of row_bytes bytes back to back at src + i * src_stride (the batch's own buffer: its pitch is its row bytes), into
// dst + i * dst_stride.  Every row gets its bytes and nothing else: pitch padding, the space between planes and pictures stay as they are.
//   PACKED: row r at dst_pitch * r.  A lane moves 16 bytes: one 16-byte load, one 16-byte store at the caller's pitch (a multiple of 16, as dst and dst_stride are).
//     Rows that are no multiple of 16 bytes long (RG24 of RGB 4:4:4 samples: 3 x width, a multiple of 4 at the least) start on longword boundaries in the batch's
//     buffer: their 16-byte pieces are loaded longword by longword, and the bytes behind the last piece leave as longwords, then bytes.
//   PLANAR_*: RG48 pictures of `width` pixels (row_bytes = 6 x width).  Plane c (R, G, B) at dst_pitch * rows * c, row r of it at dst_pitch * r, `width` elements.
//     A lane takes 8 pixels: three 16-byte loads -- 48 bytes a lane, a wave reads 3 KB of the row without a gap --, the components separated in registers (v_perm: the
//     words 3 k + c of the 24), one 16-byte store per plane for u16 / f16, two for f32 -- every store instruction of a wave writes consecutive 16-byte pieces of a plane
//     row.  The widths the RG48 gates admit are multiples of 8 but for the half-resolution pictures of RGB 4:4:4 samples (width / 2, a multiple of 4): every second
//     row of such a picture starts off a 16-byte boundary, and the whole picture goes element by element (2-byte loads, 2- or 4-byte stores; correct, slow, its rate
//     not measured).  The element loop also takes the columns behind the last whole group of eight of an aligned picture, should a gate ever admit such a width.
// No LDS, no scratch.  A wave owns a row at a time: grid (row pieces, pictures), DEC_DELIVER_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
enum { DEC_DELIVER_THREADS = 256, DEC_DELIVER_WAVES = DEC_DELIVER_THREADS / 64, DEC_DELIVER_SPLIT = 32 };
inline unsigned dec_deliver_pieces(int rows) { const int p = (rows + DEC_DELIVER_WAVES - 1) / DEC_DELIVER_WAVES; return (unsigned)(p < 1 ? 1 : (p > DEC_DELIVER_SPLIT ? DEC_DELIVER_SPLIT : p)); }

__global__ void __launch_bounds__(DEC_DELIVER_THREADS) k_dec_deliver(const uint8_t *src, size_t src_stride, int row_bytes, int rows, int width, uint8_t *dst, size_t dst_stride, int dst_pitch, int layout)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *pic = src + src_stride * (size_t)blockIdx.y;
	uint8_t *out = dst + dst_stride * (size_t)blockIdx.y;
	const bool rows_aligned = !(((uintptr_t)src | src_stride | (size_t)row_bytes) & 15);      // every row of the batch's pictures starts on a 16-byte boundary
	for (int r = (int)blockIdx.x * DEC_DELIVER_WAVES + wave; r < rows; r += (int)gridDim.x * DEC_DELIVER_WAVES) {
		const uint8_t *row = pic + (size_t)r * row_bytes;
		if (layout == DELIVER_PACKED) {
			uint8_t *orow = out + (size_t)r * dst_pitch;
			const int whole = row_bytes & ~15;
			for (int x = 16 * lane; x < whole; x += 16 * 64) {
				const cfhd_u4 v = rows_aligned ? CFHD_LDG128(row + x) : deliver_load_dword_aligned(row + x);
				store_u32x4_global(orow + x, v.x, v.y, v.z, v.w);
			}
			if (!rows_aligned) {                                     // the tail: up to three longwords, then up to three bytes
				const int words_end = row_bytes & ~3;
				for (int x = whole + 4 * lane; x < words_end; x += 4 * 64) *(uint32_t *)(orow + x) = CFHD_LDG32(row + x);
				for (int x = words_end + lane; x < row_bytes; x += 64) orow[x] = row[x];
			}
			continue;
		}
		const int elt = layout == DELIVER_PLANAR_F32 ? 4 : 2;
		const size_t plane = (size_t)dst_pitch * (size_t)rows;
		uint8_t *orow = out + (size_t)r * dst_pitch;
		const int groups = rows_aligned ? width >> 3 : 0;          // (width % 8 = 4: every second row starts off a 16-byte boundary; those pictures go element by element)
		for (int g = lane; g < groups; g += 64) {
			const cfhd_u4 a = CFHD_LDG128(row + 48 * g), b = CFHD_LDG128(row + 48 * g + 16), c = CFHD_LDG128(row + 48 * g + 32);
			// the 12 longwords hold the words R0 G0 | B0 R1 | G1 B1 of every pair of pixels
			uint8_t *at = orow + (size_t)g * 8 * elt;
			deliver_store_plane(at, deliver_lo_hi(a.x, a.y), deliver_lo_hi(a.w, b.x), deliver_lo_hi(b.z, b.w), deliver_lo_hi(c.y, c.z), layout);
			deliver_store_plane(at + plane, deliver_hi_lo(a.x, a.z), deliver_hi_lo(a.w, b.y), deliver_hi_lo(b.z, c.x), deliver_hi_lo(c.y, c.w), layout);
			deliver_store_plane(at + 2 * plane, deliver_lo_hi(a.y, a.z), deliver_lo_hi(b.x, b.y), deliver_lo_hi(b.w, c.x), deliver_lo_hi(c.z, c.w), layout);
		}
		for (int x = 8 * groups + lane; x < width; x += 64) {
			const uint16_t *px = (const uint16_t *)row + 3 * x;
			deliver_store_element(orow, x, px[0], layout);
			deliver_store_element(orow + plane, x, px[1], layout);
			deliver_store_element(orow + 2 * plane, x, px[2], layout);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// k_dec_deliver_bayer: BYR4 picture i of the pass -- the mosaic, 2 x quad_rows rows of 2 x width photosites (4 x width bytes) back to back at src + i * src_stride --
// into dst + i * dst_stride as four planes of quad_rows rows of `width` elements: plane k = 2 * (row & 1) + (column & 1) holds the photosites at that position of every
// 2 x 2 quad (red-green phase: R, G1, G2, B -- the rows r g1 / g2 b of k_inv_bayer_strip).  Plane k at dst_pitch * quad_rows * k, row q of it at dst_pitch * q.  Every
// plane row gets its bytes and nothing else.  `layout`: the element type as DELIVER_PLANAR_U16 / _F16 / _F32 (deliver_bayer_element), the element rules those of
// deliver_store_plane.
//   A wave owns a quad row at a time, two mosaic rows.  A lane takes 8 quads: two 16-byte loads from the even mosaic row and two from the odd one -- 32 consecutive
//   bytes of each row per lane, a wave reads 2 KB of each row without a gap --, the even and the odd words of each row separated in registers (v_perm_b32: 8 per
//   mosaic row, 16 per lane and step), one 16-byte store per plane for u16 / f16, two for f32 -- every store instruction of a wave writes consecutive pieces of one
//   plane row.  Every Bayer plan has component planes of whole groups of eight (build_frame_plan in cfhd_tables.cpp admits no other width), the batch's pictures come
//   from hipMalloc and lie 8 x width x quad_rows apart, and the entry point admits only pointers, strides and pitches that are multiples of 16 (checked where the
//   layout is set): every row on either side starts on a 16-byte boundary.  There is no element-by-element path.
// No LDS, no scratch.  Grid (pieces of quad rows: dec_deliver_pieces(quad_rows), pictures), DEC_DELIVER_WAVES quad rows per piece and step.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DEC_DELIVER_THREADS) k_dec_deliver_bayer(const uint8_t *src, size_t src_stride, int quad_rows, int width, uint8_t *dst, size_t dst_stride, int dst_pitch, int layout)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *pic = src + src_stride * (size_t)blockIdx.y;
	uint8_t *out = dst + dst_stride * (size_t)blockIdx.y;
	const int elt = layout == DELIVER_PLANAR_F32 ? 4 : 2, groups = width >> 3;
	const size_t plane = (size_t)dst_pitch * (size_t)quad_rows;
	for (int q = (int)blockIdx.x * DEC_DELIVER_WAVES + wave; q < quad_rows; q += (int)gridDim.x * DEC_DELIVER_WAVES) {
		const uint8_t *even = pic + (size_t)q * 8 * width, *odd = even + (size_t)4 * width;
		uint8_t *orow = out + (size_t)q * dst_pitch;
		for (int g = lane; g < groups; g += 64) {
			const cfhd_u4 a = CFHD_LDG128(even + 32 * g), b = CFHD_LDG128(even + 32 * g + 16), c = CFHD_LDG128(odd + 32 * g), d = CFHD_LDG128(odd + 32 * g + 16);
			// every longword holds the photosites of one quad row of a quad: positions 0 1 of the even mosaic row, 2 3 of the odd one
			uint8_t *at = orow + (size_t)g * 8 * elt;
			deliver_store_plane(at, deliver_lo_lo(a.x, a.y), deliver_lo_lo(a.z, a.w), deliver_lo_lo(b.x, b.y), deliver_lo_lo(b.z, b.w), layout);
			deliver_store_plane(at + plane, deliver_hi_hi(a.x, a.y), deliver_hi_hi(a.z, a.w), deliver_hi_hi(b.x, b.y), deliver_hi_hi(b.z, b.w), layout);
			deliver_store_plane(at + 2 * plane, deliver_lo_lo(c.x, c.y), deliver_lo_lo(c.z, c.w), deliver_lo_lo(d.x, d.y), deliver_lo_lo(d.z, d.w), layout);
			deliver_store_plane(at + 3 * plane, deliver_hi_hi(c.x, c.y), deliver_hi_hi(c.z, c.w), deliver_hi_hi(d.x, d.y), deliver_hi_hi(d.z, d.w), layout);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// k_dec_deliver_yuv422: packed 4:2:2 picture i of the pass -- `rows` rows of `width` pixels back to back at src + i * src_stride, 2 x width bytes a row (order
// YUV422_YUY2: Y0 U Y1 V, YUV422_2VUY: U Y0 V Y1) or 4 x width (YUV422_YU64: the words Y0 Cr Y1 Cb) -- into dst + i * dst_stride as three planes, the I422 convention:
// Y, `rows` rows of `width` elements dst_pitch bytes apart, at 0; Cb, `rows` rows of width / 2 elements dst_pitch / 2 bytes apart, at rows * dst_pitch; Cr, the same,
// behind it.  Every plane row gets its bytes and nothing else.  `layout`: DELIVER_YUV422_U8 (the bytes of an 8-bit picture as they are), _U16 (the words of YU64), _F16 /
// _F32 (deliver_unit_f32_of with the unit of the picture's own word, 255 or 65535; F16: deliver_f16_bits of it).
//   A wave owns a row at a time; a lane takes deliver_yuv422_pixels<layout> pixels, 16-byte loads of consecutive bytes, and a wave reads its stretch of the row
//   without a gap.  U8: 32 pixels, four loads (64 bytes); luma and chroma separated in registers (v_perm_b32: six per load), two 16-byte stores of luma and one
//   16-byte store per chroma plane.  U16 (YU64): 16 pixels, four loads; four v_perm_b32 per load, two 16-byte stores of luma, one per chroma plane.  F16: 16 pixels,
//   two loads of an 8-bit row or four of a YU64 row; every byte converted straight out of its longword (v_cvt_f32_ubyte0 .. 3; YU64: the words out of the halves of
//   their longwords), one multiply, v_cvt_pk_f16_f32; two 16-byte stores of luma, one per chroma plane.  F32: 8 pixels, one load or two, the same conversion, two
//   16-byte stores of luma and one per chroma plane -- measured, a lane's stores to one plane row are best kept to 32 consecutive bytes (four stores of 64 bytes a
//   lane ran at 3.8 TB/s, two of 32 bytes run at the rate of the other layouts; 16 against 32 pixels a lane for U8 was measured too: DESIGN.md section 5).  Every
//   store instruction of a wave writes consecutive pieces of one plane row.
//   The widths the decode queue serves are multiples of 16 at full resolution and of 8 at half resolution: behind the last whole group a row may have groups of
//   eight pixels left (one at 16 pixels a lane, up to three at 32), which go the same way through fewer loads and narrower stores, spread over the lanes like the
//   whole groups (U8: 8 bytes of luma, a longword per chroma plane).  The batch's
//   pictures come from hipMalloc and lie rows x row bytes apart, the entry point admits only pointers and strides that are multiples of 16 and pitches that are
//   multiples of 32 (the chroma pitch: of 16), and checks the rest where the layout is set: every row on either side starts on a 16-byte boundary.
// No LDS, no scratch.  Grid (row pieces: dec_deliver_pieces(rows), pictures), DEC_DELIVER_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
// the pixels a lane takes per step, by the element type (measured: DESIGN.md section 5)
template <int LAYOUT> struct deliver_yuv422_pixels { static constexpr int value = LAYOUT == DELIVER_YUV422_U8 ? 32 : (LAYOUT == DELIVER_YUV422_F32 ? 8 : 16); };

// K longwords at `at`: 16-byte stores (at: a multiple of 16), one 8-byte store, one longword
template <int K> __device__ __forceinline__ void deliver_store_longwords(uint8_t *at, const uint32_t *d)
{
	if constexpr (K >= 4) { for (int k = 0; k < K; k += 4) store_u32x4_global(at + 4 * k, d[k], d[k + 1], d[k + 2], d[k + 3]); }
	else if constexpr (K == 2) store_u32x2_dword_aligned((uint32_t *)at, d[0], d[1]);
	else *(uint32_t *)at = d[0];
}
// N values of the F32 rule as the elements of LAYOUT (F32: the singles; F16: deliver_f16_bits, two to a longword)
template <int LAYOUT, int N> __device__ __forceinline__ void deliver_store_floats(uint8_t *at, const float *f)
{
	if constexpr (LAYOUT == DELIVER_YUV422_F32) {
		uint32_t d[N];
		for (int k = 0; k < N; k++) memcpy(&d[k], &f[k], 4);
		deliver_store_longwords<N>(at, d);
	} else {
		uint32_t d[N / 2];
		for (int k = 0; k < N / 2; k++) d[k] = deliver_f16_bits(f[2 * k]) | (deliver_f16_bits(f[2 * k + 1]) << 16);
		deliver_store_longwords<N / 2>(at, d);
	}
}
// N pixels (8 or a multiple of 16) of an 8-bit row, 2 N bytes at `in`, to their places in the three plane rows
template <int ORDER, int LAYOUT, int N> __device__ __forceinline__ void deliver_yuv422_bytes(const uint8_t *in, uint8_t *y, uint8_t *cb, uint8_t *cr)
{
	uint32_t p[N / 2];                                           // a longword per pair of pixels
	for (int k = 0; k < N / 8; k++) { const cfhd_u4 v = CFHD_LDG128(in + 16 * k); p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w; }
	if constexpr (LAYOUT == DELIVER_YUV422_U8) {
		// of two longwords (a: bytes 0 .. 3, b: 4 .. 7 of the selector) the four luma bytes, and the chroma bytes as Cb Cb Cr Cr
		constexpr uint32_t sel_y = ORDER == YUV422_YUY2 ? 0x06040200u : 0x07050301u, sel_c = ORDER == YUV422_YUY2 ? 0x07030501u : 0x06020400u;
		uint32_t yy[N / 4], u[N / 8], v[N / 8];
		for (int k = 0; k < N / 8; k++) {
			yy[2 * k] = byte_perm(p[4 * k + 1], p[4 * k], sel_y); yy[2 * k + 1] = byte_perm(p[4 * k + 3], p[4 * k + 2], sel_y);
			const uint32_t c01 = byte_perm(p[4 * k + 1], p[4 * k], sel_c), c23 = byte_perm(p[4 * k + 3], p[4 * k + 2], sel_c);
			u[k] = deliver_lo_lo(c01, c23); v[k] = deliver_hi_hi(c01, c23);
		}
		deliver_store_longwords<N / 4>(y, yy); deliver_store_longwords<N / 8>(cb, u); deliver_store_longwords<N / 8>(cr, v);
	} else {
		constexpr int Y0 = ORDER == YUV422_YUY2 ? 0 : 8, CB = ORDER == YUV422_YUY2 ? 8 : 0;      // the bit positions of Y0 and Cb in the longword; Y1 and Cr: 16 further
		float yf[N], uf[N / 2], vf[N / 2];
		for (int j = 0; j < N / 2; j++) {
			yf[2 * j] = deliver_unit_f32_of<255>((p[j] >> Y0) & 0xffu); yf[2 * j + 1] = deliver_unit_f32_of<255>((p[j] >> (Y0 + 16)) & 0xffu);
			uf[j] = deliver_unit_f32_of<255>((p[j] >> CB) & 0xffu); vf[j] = deliver_unit_f32_of<255>((p[j] >> (CB + 16)) & 0xffu);
		}
		deliver_store_floats<LAYOUT, N>(y, yf); deliver_store_floats<LAYOUT, N / 2>(cb, uf); deliver_store_floats<LAYOUT, N / 2>(cr, vf);
	}
}
// N pixels (a multiple of 8) of a YU64 row, 4 N bytes at `in`: the longwords (Y0, Cr), (Y1, Cb) of every pair of pixels
template <int LAYOUT, int N> __device__ __forceinline__ void deliver_yuv422_words(const uint8_t *in, uint8_t *y, uint8_t *cb, uint8_t *cr)
{
	uint32_t p[N];
	for (int k = 0; k < N / 4; k++) { const cfhd_u4 v = CFHD_LDG128(in + 16 * k); p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w; }
	if constexpr (LAYOUT == DELIVER_YUV422_U16) {
		uint32_t yy[N / 2], u[N / 4], v[N / 4];
		for (int k = 0; k < N / 4; k++) {
			yy[2 * k] = deliver_lo_lo(p[4 * k], p[4 * k + 1]); yy[2 * k + 1] = deliver_lo_lo(p[4 * k + 2], p[4 * k + 3]);
			v[k] = deliver_hi_hi(p[4 * k], p[4 * k + 2]); u[k] = deliver_hi_hi(p[4 * k + 1], p[4 * k + 3]);
		}
		deliver_store_longwords<N / 2>(y, yy); deliver_store_longwords<N / 4>(cb, u); deliver_store_longwords<N / 4>(cr, v);
	} else {
		float yf[N], uf[N / 2], vf[N / 2];
		for (int j = 0; j < N / 2; j++) {
			yf[2 * j] = deliver_unit_f32_of<65535>(p[2 * j] & 0xffffu); yf[2 * j + 1] = deliver_unit_f32_of<65535>(p[2 * j + 1] & 0xffffu);
			vf[j] = deliver_unit_f32_of<65535>(p[2 * j] >> 16); uf[j] = deliver_unit_f32_of<65535>(p[2 * j + 1] >> 16);
		}
		deliver_store_floats<LAYOUT, N>(y, yf); deliver_store_floats<LAYOUT, N / 2>(cb, uf); deliver_store_floats<LAYOUT, N / 2>(cr, vf);
	}
}
// one row of `width` pixels
template <int ORDER, int LAYOUT> __device__ __forceinline__ void deliver_yuv422_row(const uint8_t *row, int width, uint8_t *y, uint8_t *cb, uint8_t *cr, int lane)
{
	constexpr int E = LAYOUT == DELIVER_YUV422_U8 ? 1 : (LAYOUT == DELIVER_YUV422_F32 ? 4 : 2);
	constexpr int P = deliver_yuv422_pixels<LAYOUT>::value;
	const int groups = width / P, units = width >> 3;            // (every width served is a multiple of 8)
	// whole groups, then the groups of eight behind the last whole one (P = 16: one, in half-resolution pictures; P = 32: up to three; P = 8: none)
	if constexpr (ORDER == YUV422_YU64) {
		for (int g = lane; g < groups; g += 64) deliver_yuv422_words<LAYOUT, P>(row + 4 * P * g, y + P * E * g, cb + (P / 2) * E * g, cr + (P / 2) * E * g);
		for (int u = groups * (P / 8) + lane; u < units; u += 64) deliver_yuv422_words<LAYOUT, 8>(row + 32 * u, y + 8 * E * u, cb + 4 * E * u, cr + 4 * E * u);
	} else {
		for (int g = lane; g < groups; g += 64) deliver_yuv422_bytes<ORDER, LAYOUT, P>(row + 2 * P * g, y + P * E * g, cb + (P / 2) * E * g, cr + (P / 2) * E * g);
		for (int u = groups * (P / 8) + lane; u < units; u += 64) deliver_yuv422_bytes<ORDER, LAYOUT, 8>(row + 16 * u, y + 8 * E * u, cb + 4 * E * u, cr + 4 * E * u);
	}
}

__global__ void __launch_bounds__(DEC_DELIVER_THREADS) k_dec_deliver_yuv422(const uint8_t *src, size_t src_stride, int rows, int width, uint8_t *dst, size_t dst_stride, int dst_pitch, int layout, int order)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *pic = src + src_stride * (size_t)blockIdx.y;
	uint8_t *out = dst + dst_stride * (size_t)blockIdx.y;
	const int row_bytes = (order == YUV422_YU64 ? 4 : 2) * width, chroma_pitch = dst_pitch >> 1;
	uint8_t *cb_plane = out + (size_t)dst_pitch * (size_t)rows, *cr_plane = cb_plane + (size_t)chroma_pitch * (size_t)rows;
	for (int r = (int)blockIdx.x * DEC_DELIVER_WAVES + wave; r < rows; r += (int)gridDim.x * DEC_DELIVER_WAVES) {
		const uint8_t *row = pic + (size_t)r * row_bytes;
		uint8_t *y = out + (size_t)r * dst_pitch, *cb = cb_plane + (size_t)r * chroma_pitch, *cr = cr_plane + (size_t)r * chroma_pitch;
		if (order == YUV422_YU64) {
			if (layout == DELIVER_YUV422_U16) deliver_yuv422_row<YUV422_YU64, DELIVER_YUV422_U16>(row, width, y, cb, cr, lane);
			else if (layout == DELIVER_YUV422_F16) deliver_yuv422_row<YUV422_YU64, DELIVER_YUV422_F16>(row, width, y, cb, cr, lane);
			else deliver_yuv422_row<YUV422_YU64, DELIVER_YUV422_F32>(row, width, y, cb, cr, lane);
		} else if (order == YUV422_YUY2) {
			if (layout == DELIVER_YUV422_U8) deliver_yuv422_row<YUV422_YUY2, DELIVER_YUV422_U8>(row, width, y, cb, cr, lane);
			else if (layout == DELIVER_YUV422_F16) deliver_yuv422_row<YUV422_YUY2, DELIVER_YUV422_F16>(row, width, y, cb, cr, lane);
			else deliver_yuv422_row<YUV422_YUY2, DELIVER_YUV422_F32>(row, width, y, cb, cr, lane);
		} else {
			if (layout == DELIVER_YUV422_U8) deliver_yuv422_row<YUV422_2VUY, DELIVER_YUV422_U8>(row, width, y, cb, cr, lane);
			else if (layout == DELIVER_YUV422_F16) deliver_yuv422_row<YUV422_2VUY, DELIVER_YUV422_F16>(row, width, y, cb, cr, lane);
			else deliver_yuv422_row<YUV422_2VUY, DELIVER_YUV422_F32>(row, width, y, cb, cr, lane);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// k_dec_deliver_rgba: packed four-component picture i of the pass -- `rows` rows of `width` pixels back to back at src + i * src_stride, 8 x width bytes a row (order
// RGBA_B64A: the native 16-bit words A R G B) or 4 x width (RGBA_BGRA, RGBA_BGRa: the bytes B G R A) -- into dst + i * dst_stride as four planes R, G, B, A (a torch
// tensor N x 4 x H x W): plane c at dst_pitch * rows * c, row r of it at dst_pitch * r, `width` elements.  The planes have the top row first: a BGRA picture lies bottom
// row first in the batch's buffer, and plane row r is read from packed row rows - 1 - r -- an address, not a second pass.  Every plane row gets its bytes and nothing
// else.  `layout`: DELIVER_RGBA_U8 (the bytes of BGRA / BGRa as they are), _U16 (the words of b64a), _F16 / _F32 (deliver_unit_f32_of with the unit of the picture's own
// word, 255 or 65535; F16: deliver_f16_bits of it).  Alpha is a component like the others.
//   A wave owns a plane row at a time; a lane's loads are 16 bytes wide and cover consecutive bytes, a wave reads its stretch of the packed row without a gap.
//   b64a: a lane takes 8 pixels, four loads (64 bytes, 4 KB a wave); every longword holds (A, R) or (G, B) of a pixel, the components of two pixels meet in one
//   longword by v_perm_b32 (16 per lane and step); one 16-byte store per plane for u16 / f16, two for f32.
//   BGRA / BGRa, U8: 16 pixels, four loads; the 4 x 4 bytes of every four pixels are transposed in two rounds of v_perm_b32 (B G and R A of a pair of pixels, then the
//   pairs of pairs: 32 per lane and step), one 16-byte store per plane.  F16: 16 pixels, every byte converted straight out of its longword (v_cvt_f32_ubyte0 .. 3),
//   one multiply, v_cvt_pk_f16_f32, two 16-byte stores per plane.  F32: 8 pixels, two loads, two 16-byte stores per plane -- a lane's stores to one plane row kept to
//   32 consecutive bytes, as measured for k_dec_deliver_yuv422.  Every store instruction of a wave writes consecutive pieces of one plane row.
//   The widths the decode queue serves for these outputs are multiples of 4 (half resolution: 100 of 200), not always of 8 or 16: the columns behind the last whole
//   group go element by element, as in k_dec_deliver.  A packed row is 8 x width or 4 x width bytes: with a width that is a multiple of 4 every row starts on a
//   16-byte boundary (the batch's pictures come from hipMalloc and lie rows x row bytes apart; the entry point checks that and admits only pointers, strides and
//   pitches that are multiples of 16).  Should a gate ever admit another width, the rows of that picture are not aligned and the whole picture goes element by element.
// No LDS, no scratch.  Grid (row pieces: dec_deliver_pieces(rows), pictures), DEC_DELIVER_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
// (CFHD_AMD_PICTURES_RGBA_*) and the packed orders they are written from
enum { DELIVER_RGBA_U8 = 11, DELIVER_RGBA_U16 = 12, DELIVER_RGBA_F16 = 13, DELIVER_RGBA_F32 = 14 };
enum { RGBA_B64A = 0, RGBA_BGRA = 1, RGBA_BGRa = 2 };
inline bool deliver_is_rgba(int layout) { return layout >= DELIVER_RGBA_U8 && layout <= DELIVER_RGBA_F32; }
inline int deliver_rgba_element_bytes(int layout) { return layout == DELIVER_RGBA_U8 ? 1 : (layout == DELIVER_RGBA_F32 ? 4 : 2); }
// the pixels a lane takes per step
template <int UNIT, int LAYOUT> struct deliver_rgba_pixels { static constexpr int value = UNIT == 65535 || LAYOUT == DELIVER_RGBA_F32 ? 8 : 16; };

// N values of the F32 rule as the elements of LAYOUT (F32: the singles; F16: deliver_f16_bits, two to a longword)
template <int LAYOUT, int N> __device__ __forceinline__ void deliver_rgba_floats(uint8_t *at, const float *f)
{
	if constexpr (LAYOUT == DELIVER_RGBA_F32) {
		uint32_t d[N];
		for (int k = 0; k < N; k++) memcpy(&d[k], &f[k], 4);
		deliver_store_longwords<N>(at, d);
	} else {
		uint32_t d[N / 2];
		for (int k = 0; k < N / 2; k++) d[k] = deliver_f16_bits(f[2 * k]) | (deliver_f16_bits(f[2 * k + 1]) << 16);
		deliver_store_longwords<N / 2>(at, d);
	}
}
// one element of a plane (the columns behind the last whole group)
template <int LAYOUT, int UNIT> __device__ __forceinline__ void deliver_rgba_element(uint8_t *plane_row, int x, uint32_t w)
{
	if constexpr (LAYOUT == DELIVER_RGBA_U8) plane_row[x] = (uint8_t)w;
	else if constexpr (LAYOUT == DELIVER_RGBA_U16) ((uint16_t *)plane_row)[x] = (uint16_t)w;
	else if constexpr (LAYOUT == DELIVER_RGBA_F16) ((uint16_t *)plane_row)[x] = (uint16_t)deliver_f16_bits(deliver_unit_f32_of<UNIT>(w));
	else ((float *)plane_row)[x] = deliver_unit_f32_of<UNIT>(w);
}
// one row of `width` b64a pixels into row `orow` of plane R; the planes `plane` bytes apart
template <int LAYOUT> __device__ __forceinline__ void deliver_rgba_row_words(const uint8_t *row, int width, bool aligned, uint8_t *orow, size_t plane, int lane)
{
	constexpr int E = LAYOUT == DELIVER_RGBA_F32 ? 4 : 2;
	const int groups = aligned ? width >> 3 : 0;
	for (int g = lane; g < groups; g += 64) {
		uint32_t p[16];                                          // (A, R), (G, B) of every pixel
		for (int k = 0; k < 4; k++) { const cfhd_u4 v = CFHD_LDG128(row + 64 * (size_t)g + 16 * k); p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w; }
		uint32_t c[4][4];                                        // plane R, G, B, A: two pixels to a longword
		for (int k = 0; k < 4; k++) {
			c[3][k] = deliver_lo_lo(p[4 * k], p[4 * k + 2]); c[0][k] = deliver_hi_hi(p[4 * k], p[4 * k + 2]);
			c[1][k] = deliver_lo_lo(p[4 * k + 1], p[4 * k + 3]); c[2][k] = deliver_hi_hi(p[4 * k + 1], p[4 * k + 3]);
		}
		uint8_t *at = orow + (size_t)g * 8 * E;
		for (int q = 0; q < 4; q++) {
			if constexpr (LAYOUT == DELIVER_RGBA_U16) store_u32x4_global(at + q * plane, c[q][0], c[q][1], c[q][2], c[q][3]);
			else {
				float f[8];
				for (int k = 0; k < 4; k++) { f[2 * k] = deliver_unit_f32_of<65535>(c[q][k] & 0xffffu); f[2 * k + 1] = deliver_unit_f32_of<65535>(c[q][k] >> 16); }
				deliver_rgba_floats<LAYOUT, 8>(at + q * plane, f);
			}
		}
	}
	for (int x = 8 * groups + lane; x < width; x += 64) {
		const uint16_t *px = (const uint16_t *)row + 4 * (size_t)x;
		deliver_rgba_element<LAYOUT, 65535>(orow + 3 * plane, x, px[0]);
		deliver_rgba_element<LAYOUT, 65535>(orow, x, px[1]);
		deliver_rgba_element<LAYOUT, 65535>(orow + plane, x, px[2]);
		deliver_rgba_element<LAYOUT, 65535>(orow + 2 * plane, x, px[3]);
	}
}
// ... and of B G R A bytes
template <int LAYOUT> __device__ __forceinline__ void deliver_rgba_row_bytes(const uint8_t *row, int width, bool aligned, uint8_t *orow, size_t plane, int lane)
{
	constexpr int E = LAYOUT == DELIVER_RGBA_U8 ? 1 : (LAYOUT == DELIVER_RGBA_F32 ? 4 : 2), P = deliver_rgba_pixels<255, LAYOUT>::value;
	const int groups = aligned ? width / P : 0;
	for (int g = lane; g < groups; g += 64) {
		uint32_t p[P];                                           // a longword per pixel: B | G << 8 | R << 16 | A << 24
		for (int k = 0; k < P / 4; k++) { const cfhd_u4 v = CFHD_LDG128(row + 4 * P * (size_t)g + 16 * k); p[4 * k] = v.x; p[4 * k + 1] = v.y; p[4 * k + 2] = v.z; p[4 * k + 3] = v.w; }
		uint8_t *at = orow + (size_t)g * P * E;
		if constexpr (LAYOUT == DELIVER_RGBA_U8) {
			uint32_t b[P / 4], gr[P / 4], r[P / 4], a[P / 4];
			for (int k = 0; k < P / 4; k++) {
				// of two pixels B0 B1 G0 G1 and R0 R1 A0 A1, then the like halves of two such pairs
				const uint32_t bg01 = byte_perm(p[4 * k + 1], p[4 * k], 0x05010400u), ra01 = byte_perm(p[4 * k + 1], p[4 * k], 0x07030602u);
				const uint32_t bg23 = byte_perm(p[4 * k + 3], p[4 * k + 2], 0x05010400u), ra23 = byte_perm(p[4 * k + 3], p[4 * k + 2], 0x07030602u);
				b[k] = deliver_lo_lo(bg01, bg23); gr[k] = deliver_hi_hi(bg01, bg23); r[k] = deliver_lo_lo(ra01, ra23); a[k] = deliver_hi_hi(ra01, ra23);
			}
			deliver_store_longwords<P / 4>(at, r); deliver_store_longwords<P / 4>(at + plane, gr); deliver_store_longwords<P / 4>(at + 2 * plane, b); deliver_store_longwords<P / 4>(at + 3 * plane, a);
		} else {
			for (int q = 0; q < 4; q++) {                          // plane q: R (bits 16), G (8), B (0), A (24)
				const int shift = q == 0 ? 16 : (q == 1 ? 8 : (q == 2 ? 0 : 24));
				float f[P];
				for (int k = 0; k < P; k++) f[k] = deliver_unit_f32_of<255>((p[k] >> shift) & 0xffu);
				deliver_rgba_floats<LAYOUT, P>(at + q * plane, f);
			}
		}
	}
	for (int x = P * groups + lane; x < width; x += 64) {
		const uint8_t *px = row + 4 * (size_t)x;
		deliver_rgba_element<LAYOUT, 255>(orow + 2 * plane, x, px[0]);
		deliver_rgba_element<LAYOUT, 255>(orow + plane, x, px[1]);
		deliver_rgba_element<LAYOUT, 255>(orow, x, px[2]);
		deliver_rgba_element<LAYOUT, 255>(orow + 3 * plane, x, px[3]);
	}
}

__global__ void __launch_bounds__(DEC_DELIVER_THREADS) k_dec_deliver_rgba(const uint8_t *src, size_t src_stride, int rows, int width, uint8_t *dst, size_t dst_stride, int dst_pitch, int layout, int order)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *pic = src + src_stride * (size_t)blockIdx.y;
	uint8_t *out = dst + dst_stride * (size_t)blockIdx.y;
	const int row_bytes = (order == RGBA_B64A ? 8 : 4) * width;
	const bool aligned = !(((uintptr_t)src | src_stride | (size_t)row_bytes) & 15);      // every row of the batch's pictures starts on a 16-byte boundary
	const size_t plane = (size_t)dst_pitch * (size_t)rows;
	for (int r = (int)blockIdx.x * DEC_DELIVER_WAVES + wave; r < rows; r += (int)gridDim.x * DEC_DELIVER_WAVES) {
		const uint8_t *row = pic + (size_t)(order == RGBA_BGRA ? rows - 1 - r : r) * row_bytes;
		uint8_t *orow = out + (size_t)r * dst_pitch;
		if (order == RGBA_B64A) {
			if (layout == DELIVER_RGBA_U16) deliver_rgba_row_words<DELIVER_RGBA_U16>(row, width, aligned, orow, plane, lane);
			else if (layout == DELIVER_RGBA_F16) deliver_rgba_row_words<DELIVER_RGBA_F16>(row, width, aligned, orow, plane, lane);
			else deliver_rgba_row_words<DELIVER_RGBA_F32>(row, width, aligned, orow, plane, lane);
		} else {
			if (layout == DELIVER_RGBA_U8) deliver_rgba_row_bytes<DELIVER_RGBA_U8>(row, width, aligned, orow, plane, lane);
			else if (layout == DELIVER_RGBA_F16) deliver_rgba_row_bytes<DELIVER_RGBA_F16>(row, width, aligned, orow, plane, lane);
			else deliver_rgba_row_bytes<DELIVER_RGBA_F32>(row, width, aligned, orow, plane, lane);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// k_dec_deliver_rgb_as_yuv: RG48 picture i of the pass -- the decoded picture of an RGB 4:4:4 or RGBA 4:4:4:4 sample, `rows` rows of `width` pixels (an even number)
// back to back at src + i * src_stride, 6 x width bytes a row -- into dst + i * dst_stride as the YU64 picture the reference decoder gives for the same sample
// (ReconstructSampleFrameRGB444ToBuffer -> TransformInverseRGB444ToYU64, decoder.c:26874, wavelet.c:4515; the arithmetic is the scalar loop of
// ConvertPlanarRGB16uToPackedYU64, convert.c:7841-7864, restated):
//   pixels (2 k, 2 k + 1) of a row form a pair.  With the RG48 words r, g, b as IEEE singles, every product and sum rounded to single on its own (no fused
//   multiply-add), evaluated as (cr * R + cg * G) + cb * B, every coefficient (float)c * 64.0f, the conversion to int truncating toward zero and >> arithmetic:
//     Y(x)  = sat16(((int)(yr r + yg g + yb b) >> 6) + 4096)
//     Cb(k) = sat16(((int)(ur (r0 + r1) + ug (g0 + g1) + ub (b0 + b1)) >> 7) + 32768), Cr(k) the same with the v row; the sums are converted to single once.
//   4096 is added under both matrices, as the reference adds it; bright pixels saturate under the video-systems one.
//   The matrix rows (y; u; v) follow bit 2 of the colour-space tag of the picture's own sample (RGB_AS_YUV_CG: the tag absent or the bit clear; RGB_AS_YUV_VS: set).
// `layout`: DELIVER_RGB_AS_YU64 -- row r at dst_pitch * r, 4 x width bytes, the words Y0 Cr Y1 Cb of every pair -- or DELIVER_RGB_AS_YUV422_U16 / _F16 / _F32: the same
// values in the geometry of k_dec_deliver_yuv422 (Y, `rows` rows of `width` elements dst_pitch apart, at 0; Cb, `rows` rows of width / 2 elements dst_pitch / 2 apart,
// behind it; Cr behind that), U16 the word, F32 deliver_unit_f32 of it, F16 deliver_f16_bits of that.  Every row gets its bytes and nothing else.
// The picture's mode: `mode` (RGB_AS_YUV_CG, _VS, or _ZERO: zeros, 0.0, in place of the picture -- a sample that failed), one for the launch; where `verdicts` is not
// null -- the launch of a pass, behind k_dec_blank, first picture 0 -- picture i has `mode` if verdicts[i] == clean and marks[i] == 0, k_dec_blank's own condition, and
// RGB_AS_YUV_ZERO otherwise (black RG48 is not zero in YU64: a blanked picture has to be told from a black one).
//   A wave owns a row at a time.  A lane holds whole pairs, no lane needs another's words: U16 / F16 16 pixels -- six 16-byte loads of consecutive bytes (96 bytes, 6 KB
//   a wave), two 16-byte stores of luma, one per chroma plane --, F32 and YU64 8 pixels -- three loads; F32 two stores of luma and one per chroma plane, YU64 two stores
//   of the packed row: a lane's stores to one row kept to 32 consecutive bytes, as measured for k_dec_deliver_yuv422.  The pairs behind the last whole group go pair by
//   pair, a lane a pair: three longword loads, and stores no wider than the pair (k_half_packed16's lesson: nothing is written behind the row bytes).  The widths the
//   encoders give RGB samples are multiples of 8: every row of the batch's buffer starts on a 16-byte boundary (checked where the layout is set); should a gate ever
//   admit an even width that is no multiple of 8, the rows are longword aligned and the whole picture goes pair by pair.
// No LDS, no scratch.  Grid (row pieces: dec_deliver_pieces(rows), pictures), DEC_DELIVER_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
// (CFHD_AMD_PICTURES_RGB_AS_*)
enum { DELIVER_RGB_AS_YU64 = 15, DELIVER_RGB_AS_YUV422_U16 = 16, DELIVER_RGB_AS_YUV422_F16 = 17, DELIVER_RGB_AS_YUV422_F32 = 18 };
enum { RGB_AS_YUV_CG = 0, RGB_AS_YUV_VS = 1, RGB_AS_YUV_ZERO = 2 };
inline bool deliver_is_rgb_as_yuv(int layout) { return layout >= DELIVER_RGB_AS_YU64 && layout <= DELIVER_RGB_AS_YUV422_F32; }
inline int deliver_rgb_as_yuv_element_bytes(int layout) { return layout == DELIVER_RGB_AS_YUV422_F32 ? 4 : 2; }
// the mode of a sample that decoded, by its colour-space tag (0: no tag)
inline int deliver_rgb_as_yuv_mode(int color_space) { return color_space & 4 ? RGB_AS_YUV_VS : RGB_AS_YUV_CG; }
template <int LAYOUT> struct deliver_rgb_as_yuv_pixels { static constexpr int value = LAYOUT == DELIVER_RGB_AS_YUV422_U16 || LAYOUT == DELIVER_RGB_AS_YUV422_F16 ? 16 : 8; };

// one product, one sum: rounded to single each, never fused.  (hipcc contracts a * b + c into a fused multiply-add by default, and through __fmul_rn / __fadd_rn too,
// which are plain operators in its headers: the pragma takes the permission away from the operations of these two functions, wherever they are inlined.  A host
// compiler for x86-64 without -mfma has no fused instruction to contract into.)
__host__ __device__ inline float deliver_mul(float a, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	return a * b;
}
__host__ __device__ inline float deliver_add(float a, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	return a + b;
}
struct RgbAsYuvMatrix { float yr, yg, yb, ur, ug, ub, vr, vg, vb; };
__host__ __device__ inline RgbAsYuvMatrix deliver_rgb_as_yuv_matrix(bool vs)
{
	RgbAsYuvMatrix m;
	m.yr = (vs ? 0.213f : 0.183f) * 64.0f; m.yg = (vs ? 0.715f : 0.614f) * 64.0f; m.yb = (vs ? 0.072f : 0.062f) * 64.0f;
	m.ur = (vs ? -0.117f : -0.101f) * 64.0f; m.ug = (vs ? -0.394f : -0.338f) * 64.0f; m.ub = (vs ? 0.511f : 0.439f) * 64.0f;
	m.vr = (vs ? 0.511f : 0.439f) * 64.0f; m.vg = (vs ? -0.464f : -0.399f) * 64.0f; m.vb = (vs ? -0.047f : -0.040f) * 64.0f;
	return m;
}
__host__ __device__ inline uint32_t deliver_sat16(int v) { return (uint32_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v)); }
__host__ __device__ inline int deliver_rgb_dot(float cr, float cg, float cb, float r, float g, float b) { return (int)deliver_add(deliver_add(deliver_mul(cr, r), deliver_mul(cg, g)), deliver_mul(cb, b)); }
// one pair of pixels, the three longwords (R0, G0), (B0, R1), (G1, B1): Y0, Y1, Cb, Cr as words
__host__ __device__ inline void deliver_rgb_as_yuv_pair(const RgbAsYuvMatrix &m, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t &y0, uint32_t &y1, uint32_t &cb, uint32_t &cr)
{
	const int r0 = (int)(d0 & 0xffffu), g0 = (int)(d0 >> 16), b0 = (int)(d1 & 0xffffu), r1 = (int)(d1 >> 16), g1 = (int)(d2 & 0xffffu), b1 = (int)(d2 >> 16);
	y0 = deliver_sat16((deliver_rgb_dot(m.yr, m.yg, m.yb, (float)r0, (float)g0, (float)b0) >> 6) + 4096);
	y1 = deliver_sat16((deliver_rgb_dot(m.yr, m.yg, m.yb, (float)r1, (float)g1, (float)b1) >> 6) + 4096);
	const float rs = (float)(r0 + r1), gs = (float)(g0 + g1), bs = (float)(b0 + b1);
	cb = deliver_sat16((deliver_rgb_dot(m.ur, m.ug, m.ub, rs, gs, bs) >> 7) + 32768);
	cr = deliver_sat16((deliver_rgb_dot(m.vr, m.vg, m.vb, rs, gs, bs) >> 7) + 32768);
}
// N words of one plane row (N: 1 or a multiple of 2) as the elements of LAYOUT at `at`
template <int LAYOUT, int N> __device__ __forceinline__ void deliver_rgb_as_yuv_store(uint8_t *at, const uint32_t *w)
{
	if constexpr (N == 1) {
		if constexpr (LAYOUT == DELIVER_RGB_AS_YUV422_F32) { const float f = deliver_unit_f32(w[0]); uint32_t d; memcpy(&d, &f, 4); *(uint32_t *)at = d; }
		else *(uint16_t *)at = (uint16_t)(LAYOUT == DELIVER_RGB_AS_YUV422_F16 ? deliver_f16_bits(deliver_unit_f32(w[0])) : w[0]);
	} else if constexpr (LAYOUT == DELIVER_RGB_AS_YUV422_F32) {
		uint32_t d[N];
		for (int k = 0; k < N; k++) { const float f = deliver_unit_f32(w[k]); memcpy(&d[k], &f, 4); }
		deliver_store_longwords<N>(at, d);
	} else {
		uint32_t d[N / 2];
		for (int k = 0; k < N / 2; k++)
			d[k] = LAYOUT == DELIVER_RGB_AS_YUV422_F16 ? (deliver_f16_bits(deliver_unit_f32(w[2 * k])) | (deliver_f16_bits(deliver_unit_f32(w[2 * k + 1])) << 16)) : (w[2 * k] | (w[2 * k + 1] << 16));
		deliver_store_longwords<N / 2>(at, d);
	}
}
// N pixels (2: one pair, longword loads; 8 or 16: 16-byte loads at `in`, a multiple of 16) of an RG48 row to their places: `y` the packed row (YU64) or the luma row
template <int LAYOUT, int N> __device__ __forceinline__ void deliver_rgb_as_yuv_pixels_at(const RgbAsYuvMatrix &m, bool zero, const uint8_t *in, uint8_t *y, uint8_t *cb, uint8_t *cr)
{
	uint32_t d[3 * N / 2], yy[N], u[N / 2], v[N / 2];
	if (zero) { for (int k = 0; k < N; k++) yy[k] = 0u; for (int k = 0; k < N / 2; k++) u[k] = v[k] = 0u; }
	else {
		if constexpr (N == 2) { d[0] = CFHD_LDG32(in); d[1] = CFHD_LDG32(in + 4); d[2] = CFHD_LDG32(in + 8); }
		else for (int k = 0; k < 3 * N / 8; k++) { const cfhd_u4 q = CFHD_LDG128(in + 16 * k); d[4 * k] = q.x; d[4 * k + 1] = q.y; d[4 * k + 2] = q.z; d[4 * k + 3] = q.w; }
		for (int j = 0; j < N / 2; j++) deliver_rgb_as_yuv_pair(m, d[3 * j], d[3 * j + 1], d[3 * j + 2], yy[2 * j], yy[2 * j + 1], u[j], v[j]);
	}
	if constexpr (LAYOUT == DELIVER_RGB_AS_YU64) {
		uint32_t p[N];                                           // (Y0, Cr), (Y1, Cb) of every pair
		for (int j = 0; j < N / 2; j++) { p[2 * j] = yy[2 * j] | (v[j] << 16); p[2 * j + 1] = yy[2 * j + 1] | (u[j] << 16); }
		deliver_store_longwords<N>(y, p);
	} else {
		deliver_rgb_as_yuv_store<LAYOUT, N>(y, yy); deliver_rgb_as_yuv_store<LAYOUT, N / 2>(cb, u); deliver_rgb_as_yuv_store<LAYOUT, N / 2>(cr, v);
	}
}
// one row of `width` pixels (even)
template <int LAYOUT> __device__ __forceinline__ void deliver_rgb_as_yuv_row(const RgbAsYuvMatrix &m, bool zero, const uint8_t *row, int width, bool aligned, uint8_t *y, uint8_t *cb, uint8_t *cr, int lane)
{
	constexpr int P = deliver_rgb_as_yuv_pixels<LAYOUT>::value;
	// the bytes a pixel has in the row `y` points at, and a chroma element in its plane row
	constexpr int E = LAYOUT == DELIVER_RGB_AS_YU64 || LAYOUT == DELIVER_RGB_AS_YUV422_F32 ? 4 : 2, C = LAYOUT == DELIVER_RGB_AS_YUV422_F32 ? 4 : 2;
	const int groups = aligned ? width / P : 0, pairs = width >> 1;
	for (int g = lane; g < groups; g += 64) deliver_rgb_as_yuv_pixels_at<LAYOUT, P>(m, zero, row + (size_t)6 * P * g, y + (size_t)P * E * g, cb + (size_t)(P / 2) * C * g, cr + (size_t)(P / 2) * C * g);
	for (int k = groups * (P / 2) + lane; k < pairs; k += 64) deliver_rgb_as_yuv_pixels_at<LAYOUT, 2>(m, zero, row + (size_t)12 * k, y + (size_t)2 * E * k, cb + (size_t)C * k, cr + (size_t)C * k);
}

__global__ void __launch_bounds__(DEC_DELIVER_THREADS) k_dec_deliver_rgb_as_yuv(const uint8_t *src, size_t src_stride, int rows, int width, uint8_t *dst, size_t dst_stride, int dst_pitch, int layout, int mode,
                                                                               const uint32_t *verdicts, const uint32_t *marks, uint32_t clean)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	// (the two words through the vector memory path, as everything else this kernel reads: a volatile access is never given to the scalar unit)
	if (verdicts && !(((const volatile uint32_t *)verdicts)[blockIdx.y] == clean && !((const volatile uint32_t *)marks)[blockIdx.y])) mode = RGB_AS_YUV_ZERO;
	const bool zero = mode == RGB_AS_YUV_ZERO;
	const RgbAsYuvMatrix m = deliver_rgb_as_yuv_matrix(mode == RGB_AS_YUV_VS);
	const uint8_t *pic = src + src_stride * (size_t)blockIdx.y;
	uint8_t *out = dst + dst_stride * (size_t)blockIdx.y;
	const int row_bytes = 6 * width, chroma_pitch = dst_pitch >> 1;
	const bool aligned = !(((uintptr_t)src | src_stride | (size_t)row_bytes) & 15);      // every row of the batch's pictures starts on a 16-byte boundary
	uint8_t *cb_plane = out + (size_t)dst_pitch * (size_t)rows, *cr_plane = cb_plane + (size_t)chroma_pitch * (size_t)rows;
	for (int r = (int)blockIdx.x * DEC_DELIVER_WAVES + wave; r < rows; r += (int)gridDim.x * DEC_DELIVER_WAVES) {
		const uint8_t *row = pic + (size_t)r * row_bytes;
		uint8_t *y = out + (size_t)r * dst_pitch, *cb = cb_plane + (size_t)r * chroma_pitch, *cr = cr_plane + (size_t)r * chroma_pitch;
		if (layout == DELIVER_RGB_AS_YU64) deliver_rgb_as_yuv_row<DELIVER_RGB_AS_YU64>(m, zero, row, width, aligned, y, cb, cr, lane);
		else if (layout == DELIVER_RGB_AS_YUV422_U16) deliver_rgb_as_yuv_row<DELIVER_RGB_AS_YUV422_U16>(m, zero, row, width, aligned, y, cb, cr, lane);
		else if (layout == DELIVER_RGB_AS_YUV422_F16) deliver_rgb_as_yuv_row<DELIVER_RGB_AS_YUV422_F16>(m, zero, row, width, aligned, y, cb, cr, lane);
		else deliver_rgb_as_yuv_row<DELIVER_RGB_AS_YUV422_F32>(m, zero, row, width, aligned, y, cb, cr, lane);
	}
}

// ---------------------------------------------------------------------------------------------
// k_dec_deliver_rgb10: picture i of the pass -- `rows` rows of `width` DPX0 longwords (big-endian, r << 22 | g << 12 | b << 2: the thumbnails of
// cfhd_amd_decode_batch_create_thumbnails) back to back at src + i * src_stride -- into dst + i * dst_stride as three planes R, G, B of `rows` rows of `width` elements,
// rows dst_pitch apart, planes rows x dst_pitch apart (a torch tensor N x 3 x H x W).  Every plane row gets its bytes and nothing else.  `layout`: DELIVER_RGB10_U16 (the
// 10-bit value as it is, 0 .. 1023), _F32 (deliver_unit_f32_of<1023>), _F16 (deliver_f16_bits of that): the rules of the other plane layouts with the unit of the
// picture's own word.
//   A wave owns a row at a time.  Where the row starts on a 16-byte boundary (always when 4 x width and src_stride are multiples of 16; every second row, or none, of
//   the others: decided per row, wave-uniform) a lane takes 8 pixels: two 16-byte loads -- a wave reads 2 KB of the row without a gap --, the bytes swapped and the
//   three fields separated in registers, one 16-byte store per plane for u16 / f16, two for f32.  The pixels behind the last whole group of eight, and every pixel of
//   a row that starts elsewhere (on a longword boundary: src, src_stride and 4 x width are multiples of 4), go element by element: a 4-byte load, three 2- or 4-byte
//   stores.  Nothing ties the kernel to thumbnails: width, rows and the source stride are arguments.
// No LDS, no scratch.  Grid (row pieces: dec_deliver_pieces(rows), pictures), DEC_DELIVER_WAVES rows per piece and step.
// ---------------------------------------------------------------------------------------------
enum { DELIVER_RGB10_U16 = 19, DELIVER_RGB10_F16 = 20, DELIVER_RGB10_F32 = 21 };      // (CFHD_AMD_PICTURES_RGB10_*)
inline bool deliver_is_rgb10(int layout) { return layout >= DELIVER_RGB10_U16 && layout <= DELIVER_RGB10_F32; }
inline int deliver_rgb10_element_bytes(int layout) { return layout == DELIVER_RGB10_F32 ? 4 : 2; }
// the DPX0 longword as it was loaded, in the machine's order
__device__ __forceinline__ uint32_t deliver_rgb10_word(uint32_t l) { return byte_perm(0u, l, 0x00010203u); }
// eight 10-bit values of one plane (at: a multiple of 16)
template <int LAYOUT> __device__ __forceinline__ void deliver_rgb10_store(uint8_t *at, const uint32_t *v)
{
	if constexpr (LAYOUT == DELIVER_RGB10_U16) store_u32x4_global(at, v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
	else {
		float f[8];
		for (int k = 0; k < 8; k++) f[k] = deliver_unit_f32_of<1023>(v[k]);
		deliver_store_floats<LAYOUT == DELIVER_RGB10_F32 ? DELIVER_YUV422_F32 : DELIVER_YUV422_F16, 8>(at, f);
	}
}
template <int LAYOUT> __device__ __forceinline__ void deliver_rgb10_element(uint8_t *plane_row, int x, uint32_t v)
{
	if constexpr (LAYOUT == DELIVER_RGB10_U16) ((uint16_t *)plane_row)[x] = (uint16_t)v;
	else if constexpr (LAYOUT == DELIVER_RGB10_F16) ((uint16_t *)plane_row)[x] = (uint16_t)deliver_f16_bits(deliver_unit_f32_of<1023>(v));
	else ((float *)plane_row)[x] = deliver_unit_f32_of<1023>(v);
}
template <int LAYOUT> __device__ __forceinline__ void deliver_rgb10_row(const uint8_t *row, int width, uint8_t *orow, size_t plane, int lane)
{
	constexpr int E = LAYOUT == DELIVER_RGB10_F32 ? 4 : 2;
	const int groups = ((uintptr_t)row & 15) ? 0 : width >> 3;
	for (int g = lane; g < groups; g += 64) {
		const cfhd_u4 a = CFHD_LDG128(row + 32 * (size_t)g), b = CFHD_LDG128(row + 32 * (size_t)g + 16);
		const uint32_t w[8] = { deliver_rgb10_word(a.x), deliver_rgb10_word(a.y), deliver_rgb10_word(a.z), deliver_rgb10_word(a.w),
		                        deliver_rgb10_word(b.x), deliver_rgb10_word(b.y), deliver_rgb10_word(b.z), deliver_rgb10_word(b.w) };
		uint32_t r[8], gr[8], bl[8];
		for (int k = 0; k < 8; k++) { r[k] = w[k] >> 22; gr[k] = (w[k] >> 12) & 0x3ffu; bl[k] = (w[k] >> 2) & 0x3ffu; }
		uint8_t *at = orow + (size_t)g * 8 * E;
		deliver_rgb10_store<LAYOUT>(at, r); deliver_rgb10_store<LAYOUT>(at + plane, gr); deliver_rgb10_store<LAYOUT>(at + 2 * plane, bl);
	}
	for (int x = 8 * groups + lane; x < width; x += 64) {
		const uint32_t w = deliver_rgb10_word(CFHD_LDG32(row + 4 * (size_t)x));
		deliver_rgb10_element<LAYOUT>(orow, x, w >> 22);
		deliver_rgb10_element<LAYOUT>(orow + plane, x, (w >> 12) & 0x3ffu);
		deliver_rgb10_element<LAYOUT>(orow + 2 * plane, x, (w >> 2) & 0x3ffu);
	}
}

__global__ void __launch_bounds__(DEC_DELIVER_THREADS) k_dec_deliver_rgb10(const uint8_t *src, size_t src_stride, int rows, int width, uint8_t *dst, size_t dst_stride, int dst_pitch, int layout)
{
	const int lane = (int)(threadIdx.x & 63u), wave = wave_uniform((int)(threadIdx.x >> 6));
	const uint8_t *pic = src + src_stride * (size_t)blockIdx.y;
	uint8_t *out = dst + dst_stride * (size_t)blockIdx.y;
	const size_t plane = (size_t)dst_pitch * (size_t)rows;
	for (int r = (int)blockIdx.x * DEC_DELIVER_WAVES + wave; r < rows; r += (int)gridDim.x * DEC_DELIVER_WAVES) {
		const uint8_t *row = pic + (size_t)r * 4 * (size_t)width;
		uint8_t *orow = out + (size_t)r * dst_pitch;
		if (layout == DELIVER_RGB10_U16) deliver_rgb10_row<DELIVER_RGB10_U16>(row, width, orow, plane, lane);
		else if (layout == DELIVER_RGB10_F16) deliver_rgb10_row<DELIVER_RGB10_F16>(row, width, orow, plane, lane);
		else deliver_rgb10_row<DELIVER_RGB10_F32>(row, width, orow, plane, lane);
	}
}

} // namespace dev
} // namespace cfhd
