// cfhd_ingest_kernels.h -- the two kernels of the decode queue (cfhd_decode_queue.hip) that are not the decoder's own: k_dec_ingest in front of the parser, k_dec_blank
// behind the last conversion.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <cfhd_gfx950.h>

namespace cfhd {
namespace dev {

// What k_dec_parse stores per sample when it is given a verdict table (cfhd_entropy_kernels.h): why the walk failed in the low byte (0: it did not), what the handle
// learns from the whole sample -- the progressive flag, the colour-space tag -- above it.  A clean sample of the prepared kind carries exactly dec_verdict_word(0, ...).
enum { DEC_VERDICT_OK = 0, DEC_VERDICT_MALFORMED = 1, DEC_VERDICT_GEOMETRY = 2, DEC_VERDICT_FORMAT = 3, DEC_VERDICT_BANDS = 4,
       DEC_VERDICT_HOST = 5 };      // HOST: a sample only the host parser judges (an UNCOMPRESS chunk): the slow path
__host__ __device__ inline uint32_t dec_verdict_word(int reason, int progressive, int color_space) { return (uint32_t)reason | ((uint32_t)(progressive & 1) << 8) | ((uint32_t)(color_space & 0xffff) << 16); }

// ---------------------------------------------------------------------------------------------
// k_dec_ingest: samples as a file holds them -- sample i is size[i] bytes at blob + src[i], any byte alignment, any order, gaps between them -- into the decoder's own
// slots (slot i at slots + i * slot_stride, both multiples of 256: what k_dec_parse and the band decoders read longword by longword), d_sizes[i] beside them.
// Every sample byte passes through here once: aligned 16-byte loads of the source (two per 16 bytes of output, the second one a hit in the line the first brought),
// the bytes shifted into place with v_perm (byte_perm; the shift is the same for a whole sample, so the selector and the pick of the five source words are
// wave-uniform), 16-byte stores.  The work is cut into pieces of DEC_INGEST_PIECE bytes of a slot, a workgroup each: first_piece[i] is the number of pieces in front
// of sample i (n + 1 entries, the host's running sum), a workgroup finds its sample by bisection -- one long sample and many short ones load the grid alike.
// A sample's pieces cover its bytes and the zeros behind them up to the next multiple of 256: the window the parser's last fetch reads (DecTagReader) never shows what
// an earlier pass left in the slot.  A sample longer than its slot or of a size that is no multiple of 4 is not copied: size 0, marks[i] = 1 (the caller decodes it
// elsewhere).  Nothing is read outside the 16-byte blocks that hold bytes of a sample, so nothing outside the 16-byte hull of the blob.
// Slots of two sizes (a batch of two-frame groups: a group sample's slot, and a small one for the P-frame sample behind it): the table names entry i's slot -- dst[i]
// bytes from `slots`, a multiple of 256, cap[i] bytes long, a multiple of 256 too -- instead of i * slot_stride and slot_stride.
// grid: max(1, first_piece[n]) workgroups of DEC_INGEST_THREADS.
// ---------------------------------------------------------------------------------------------
enum { DEC_INGEST_THREADS = 256, DEC_INGEST_PIECE = 16384 };      // four 16-byte vectors a lane
struct DecIngestTable { const unsigned long long *src; const uint32_t *size, *first_piece; const unsigned long long *dst; const uint32_t *cap; };      // [n], [n], [n + 1], and [n], [n] or null, in device memory

__host__ __device__ inline uint32_t dec_ingest_pieces(uint32_t size, size_t slot_stride)
{
	if ((size & 3u) || size > slot_stride) return 0u;
	return (uint32_t)((((size_t)size + 255u) & ~(size_t)255u) + DEC_INGEST_PIECE - 1) / DEC_INGEST_PIECE;
}

// the 16 bytes at byte `shift` (0 .. 15) of the 32 bytes a, b
__device__ __forceinline__ cfhd_u4 dec_ingest_shift(const cfhd_u4 a, const cfhd_u4 b, uint32_t shift)
{
	uint32_t w0, w1, w2, w3, w4;
	switch (shift >> 2) {
	case 0: w0 = a.x; w1 = a.y; w2 = a.z; w3 = a.w; w4 = b.x; break;
	case 1: w0 = a.y; w1 = a.z; w2 = a.w; w3 = b.x; w4 = b.y; break;
	case 2: w0 = a.z; w1 = a.w; w2 = b.x; w3 = b.y; w4 = b.z; break;
	default: w0 = a.w; w1 = b.x; w2 = b.y; w3 = b.z; w4 = b.w; break;
	}
	const uint32_t sel = 0x03020100u + 0x01010101u * (shift & 3u);      // bytes (shift & 3) .. (shift & 3) + 3 of the pair (low word, high word)
	cfhd_u4 r;
	r.x = byte_perm(w1, w0, sel); r.y = byte_perm(w2, w1, sel); r.z = byte_perm(w3, w2, sel); r.w = byte_perm(w4, w3, sel);
	return r;
}

__global__ void __launch_bounds__(DEC_INGEST_THREADS) k_dec_ingest(const uint8_t *blob, DecIngestTable T, int n, uint8_t *slots, size_t slot_stride, uint32_t *d_sizes, uint32_t *marks)
{
	// the size table and the marks: one entry a lane over the whole grid
	for (int i = (int)(blockIdx.x * DEC_INGEST_THREADS + threadIdx.x); i < n; i += (int)(gridDim.x * DEC_INGEST_THREADS)) {
		const uint32_t size = T.size[i];
		const bool copied = !(size & 3u) && size <= (T.cap ? (size_t)T.cap[i] : slot_stride);
		d_sizes[i] = copied ? size : 0u;
		marks[i] = copied ? 0u : 1u;
	}
	const uint32_t piece = blockIdx.x;
	if (piece >= T.first_piece[n]) return;                  // (the one workgroup of a pass without bytes)
	int lo = 0, hi = n - 1;                                  // the last sample whose first piece is not behind this one
	while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (T.first_piece[mid] <= piece) lo = mid; else hi = mid - 1; }
	const int i = wave_uniform(lo);
	const uint32_t size = T.size[i];
	const uint32_t padded = (size + 255u) & ~255u;
	const uint32_t p0 = (piece - T.first_piece[i]) * (uint32_t)DEC_INGEST_PIECE;
	const uint32_t p1 = p0 + DEC_INGEST_PIECE < padded ? p0 + DEC_INGEST_PIECE : padded;
	const unsigned long long s0 = T.src[i];
	const uint32_t shift = (uint32_t)wave_uniform((int)((uint32_t)((uintptr_t)blob + s0) & 15u));
	const uint8_t *src = blob + s0 - shift;                  // 16-byte aligned: the block that holds the sample's first byte
	uint8_t *dst = T.dst ? slots + T.dst[i] : slots + slot_stride * (size_t)i;
	const cfhd_u4 zero = { 0u, 0u, 0u, 0u };
	for (uint32_t p = p0 + 16u * threadIdx.x; p < p1; p += 16u * DEC_INGEST_THREADS) {
		cfhd_u4 v = zero;
		if (p < size) {                                     // (size and p are multiples of 4 and of 16: whole words of the vector lie on either side of the end)
			const cfhd_u4 a = CFHD_LDG128(src + p);
			// the next block only where it holds bytes of this sample
			const cfhd_u4 b = shift && p + 16u - shift < size ? CFHD_LDG128(src + p + 16u) : zero;
			v = shift ? dec_ingest_shift(a, b, shift) : a;
			if (p + 4u >= size) v.y = 0u;
			if (p + 8u >= size) v.z = 0u;
			if (p + 12u >= size) v.w = 0u;
		}
		store_u32x4_global(dst + p, v.x, v.y, v.z, v.w);
	}
}

// ---------------------------------------------------------------------------------------------
// k_dec_blank: behind the last transform launch and its conversion.  Zeroes the picture rows (row_bytes of each, nothing behind them) of every sample whose verdict is
// not the clean word of the prepared kind or that k_dec_ingest marked: a sample that failed -- or that is decoded elsewhere -- never shows the picture an earlier pass
// left in its place (CFHD_DecodeSample zero-fills on failure, decoder.c:11850-11859).  grid (DEC_BLANK_SPLIT, samples); clean samples cost one load.
// A batch of two-frame groups (followers > 0: their number of table entries in front of the followers' entries): pictures 2 g and 2 g + 1 belong to the pair of
// group g, verdicts[g] / marks[g], and its follower, verdicts[followers + g] (0: clean) / marks[followers + g]; a pair that is not clean on both sides has both zeroed.
// ---------------------------------------------------------------------------------------------
enum { DEC_BLANK_THREADS = 256, DEC_BLANK_SPLIT = 8 };
__global__ void __launch_bounds__(DEC_BLANK_THREADS) k_dec_blank(const uint32_t *verdicts, const uint32_t *marks, uint32_t clean, uint8_t *pictures, size_t picture_bytes, int pitch, int row_bytes, int rows,
                                                                 int followers = 0)
{
	const int i = blockIdx.y;
	if (followers) { const int g = i >> 1; if (verdicts[g] == clean && !marks[g] && verdicts[followers + g] == 0u && !marks[followers + g]) return; }
	else if (verdicts[i] == clean && !marks[i]) return;
	uint8_t *pic = pictures + picture_bytes * (size_t)i;
	const bool longwords = !((row_bytes | pitch | (int)(picture_bytes & 3u)) & 3);      // rows of whole longwords on a longword pitch: every output but RG24 at some widths
	for (int r = blockIdx.x; r < rows; r += DEC_BLANK_SPLIT) {
		uint8_t *row = pic + (size_t)r * pitch;
		if (longwords) for (int x = threadIdx.x; x < (row_bytes >> 2); x += DEC_BLANK_THREADS) ((uint32_t *)row)[x] = 0u;
		else for (int x = threadIdx.x; x < row_bytes; x += DEC_BLANK_THREADS) row[x] = 0u;
	}
}

} // namespace dev
} // namespace cfhd
