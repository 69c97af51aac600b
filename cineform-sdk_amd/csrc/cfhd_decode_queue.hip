// cfhd_decode_queue.hip -- the decode queue (extension API, cfhd_amd_decode_batch_*): batches of intra samples that came from anywhere -- the reference encoder, a camera,
// a file -- decoded the way the round-trip batch of cfhd_batch.cpp decodes the samples of its own coder: parsed on the GPU, one launch per stage for the whole batch,
// no host wait inside a pass.
//
// A pass on the batch's one stream:
//   (samples H2D: one DMA of a registered blob as it lies, or of the pinned buffer the calling thread packed plain memory into)  ->  k_dec_ingest: every sample into the
//   decoder's own 256-byte aligned slot, the size table  ->  k_dec_parse with a verdict per sample  ->  the band decoder, k_dec_lowpass  ->  the three transform levels
//   and the output conversion (DecodeBatch)  ->  k_dec_blank: the pictures of the samples that failed, zeroed  ->  (k_dec_deliver: the pictures into the
//   device memory cfhd_amd_decode_batch_set_device_pictures named, packed or as planes; k_dec_deliver_rgb_as_yuv: the RG48 pictures of RGB samples as the YU64
//   picture the reference decodes such a sample to, every picture with the matrix of its own sample's colour-space tag)  ->  (pictures D2H).
// The gates are the handle's: create prepares a CFHD_DecodeSample handle on the first sample and decodes that sample once; what the handle refuses, create refuses with
// the same text.  That handle stays with the batch as the slow path: the samples k_dec_ingest could not place (longer than a slot, a size that is no multiple of 4),
// those whose scan or colour-space tag differs from the first sample's, and -- when the band decoders' one error word is set after the pass -- every sample the parser
// passed get their verdict and picture from it in wait ("every caller decodes alone and gets its own verdict", as DecodeService decides).  A pass of intact samples
// launches nothing extra.
//
// A batch of two-frame groups (cfhd_amd_decode_batch_create_groups): entry 2 g of a pass is group sample g, entry 2 g + 1 the P-frame sample behind it, pictures 2 g
// and 2 g + 1 the group's two frames.  The same pass with the group decoder's parts: k_dec_ingest places group g in a slot of the handle's capacity and its follower
// in a small slot behind the group slots (the table names every entry's slot: groups in front, followers behind them)  ->  k_dec_parse_group with a verdict per
// group and per follower  ->  the band decoder (k_dec_band_two_pass for subband 7 of the groups from 8-bit RGB sources), k_dec_lowpass  ->  GopBatch's inverse
// stages  ->  k_dec_blank over pairs.  A pair is judged alone: the slow handle forgets its last group in front of every pair it is given.
//
// A batch of thumbnails (cfhd_amd_decode_batch_create_thumbnails): the 1/8 x 1/8 DPX0 picture CFHD_GetThumbnail makes of every sample, from the raw lowpass words in
// its slot.  The front of the same pass and nothing of the decoder: k_dec_ingest  ->  k_dec_parse (by itself: DecParseTables, no pyramid behind its tables)  ->
// k_dec_thumbnail, which also writes the zeros of the samples without a clean verdict  ->  (k_dec_deliver: the DPX0 words; k_dec_deliver_rgb10: three planes of the 10-bit
// values)  ->  (pictures D2H).  Such a batch never goes through DecodeBatch::prepare: it owns its slots, tables, verdicts and small pictures and one stream.  The slow
// path of wait is CFHD_GetThumbnail on the sample's bytes: the samples k_dec_ingest could not place and those the parser does not pass (low byte of the verdict 1 .. 5).
#include "../../include/cfhd_amd.h"
#include "cfhd_core.h"
#include "cfhd_bitstream.h"
#include "cfhd_device.h"
#include "cfhd_params.h"
#include "cfhd_ingest_kernels.h"
#include "cfhd_deliver_kernels.h"
#include "cfhd_thumbnail_kernels.h"
#include "cfhd_entropy_gpu.h"
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <thread>
#include <atomic>
#include <new>

using namespace cfhd;

namespace {
enum { ERR_OKAY = 0, ERR_BADSAMPLE = 5, ERR_INTERNAL = 6 };
int g_fail(hipError_t e, const char *what) { fprintf(stderr, "[cfhd_amd] %s: %s\n", what, hipGetErrorString(e)); return (int)e ? (int)e : -1; }
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return g_fail(_e, #expr); } while (0)

template <typename F> void parallel_for(int n, int nthreads, F f)
{
	if (nthreads <= 1 || n <= 1) { for (int i = 0; i < n; i++) f(i); return; }
	std::atomic<int> next(0);
	std::vector<std::thread> pool;
	for (int k = 0; k < (nthreads < n ? nthreads : n); k++) pool.emplace_back([&] { for (int i; (i = next.fetch_add(1)) < n;) f(i); });
	for (auto &th : pool) th.join();
}
}

struct cfhd_amd_decode_batch {
	int n = 0, device = 0;
	DecoderHandleState st;
	DecodeBatch dec;
	// a batch of two-frame groups: n = 2 ngroups samples, decoded by gdec; group g is table entry g, its follower entry ngroups + g (entry_of)
	bool groups = false; int ngroups = 0; GopBatch gdec; DecoderGroupState gst;
	uint8_t *d_slots = nullptr; size_t group_cap = 0; char band_name[96] = "";
	// a batch of thumbnails: thumb_w x thumb_h DPX0 longwords a picture in d_thumbs, slots of thumb_cap bytes in d_slots, k_dec_parse's own tables, the batch's one stream;
	// h_thumbs: pinned, allocated by the first pass that delivers to plain host memory (thumbs_staged: this pass does)
	bool thumbs = false; int thumb_w = 0, thumb_h = 0, thumb_yuv422 = 0; size_t thumb_cap = 0; void *thumb_stream = nullptr;
	DecParseTables parse; uint8_t *d_thumbs = nullptr, *h_thumbs = nullptr; bool thumbs_staged = false; float parse_ms = 0, thumb_ms = 0;
	enum { kFollowerCap = 1024 };            // the slot of a P-frame sample (24 bytes as the encoders write it); a longer one is the slow path's
	CFHD_DecoderRef slow = nullptr;          // the handle create prepared on the first sample: the gates, and the slow path of wait
	void *scope_stream = nullptr;            // the batch's one stream (StreamScope): released behind the decoder
	// the samples on their way in: the blob in HBM (+ the pinned buffer plain memory is packed into), the table k_dec_ingest reads, what it and the parser write
	uint8_t *d_blob = nullptr, *h_blob = nullptr; size_t blob_cap = 0;      // (h_blob: allocated by the first pass that stages plain memory)
	uint8_t *d_table = nullptr, *h_table = nullptr; size_t table_bytes = 0;
	uint32_t *d_sizes = nullptr, *d_verdicts = nullptr, *h_verdicts = nullptr;      // verdicts: [0, n) k_dec_parse's words, [n, 2 n) k_dec_ingest's marks
	hipEvent_t ev[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };    // around k_dec_ingest, around k_dec_blank, around k_dec_deliver
	float ingest_ms = 0, blank_ms = 0, deliver_ms = 0; bool timed = false, deliver_timed = false;
	// where every pass delivers its pictures on the device (cfhd_amd_decode_batch_set_device_pictures; null: nowhere): the caller's memory, borrowed from submit to wait
	uint8_t *dev_out = nullptr; size_t dev_out_stride = 0; int dev_out_pitch = 0, dev_out_layout = 0;
	// the pass in flight
	bool in_flight = false; int count = 0; uint32_t steps = 0;
	bool counted = false;                                          // ... is one of the device's passes in flight (cfhd_device.h device_pass_begin: begin_pass to end_pass)
	const uint8_t *src_host = nullptr, *src_device = nullptr;      // where sample i's bytes are for the slow path: src + offsets[i]
	std::vector<unsigned long long> offsets; std::vector<uint32_t> sizes;      // sizes: as k_dec_ingest sees them (a sample beyond 4 GB: 0xffffffff, no multiple of 4 -- the slow path's)
	std::vector<size_t> full_sizes;
	uint8_t *host_out = nullptr; size_t host_out_stride = 0; int host_out_pitch = 0;
	std::vector<std::vector<uint8_t>> slow_pictures;               // pictures the slow path decoded while the batch keeps its pictures in HBM (download_output serves them)
	unsigned long long *table_src() const { return (unsigned long long *)h_table; }
	uint32_t *table_size() const { return (uint32_t *)(h_table + 8 * (size_t)n); }
	uint32_t *table_first() const { return (uint32_t *)(h_table + 12 * (size_t)n); }
	// (groups: the entries' slots behind the intra table -- offsets from d_slots, capacities)
	size_t table_dst_at() const { return (16 * (size_t)n + 4 + 7) & ~(size_t)7; }
	unsigned long long *table_dst() const { return (unsigned long long *)(h_table + table_dst_at()); }
	uint32_t *table_cap() const { return (uint32_t *)(h_table + table_dst_at() + 8 * (size_t)n); }
	dev::DecIngestTable device_table() const
	{
		return dev::DecIngestTable{ (const unsigned long long *)d_table, (const uint32_t *)(d_table + 8 * (size_t)n), (const uint32_t *)(d_table + 12 * (size_t)n),
		                            groups ? (const unsigned long long *)(d_table + table_dst_at()) : nullptr, groups ? (const uint32_t *)(d_table + table_dst_at() + 8 * (size_t)n) : nullptr };
	}
	uint32_t clean_word() const { return dev::dec_verdict_word(0, st.progressive_flag, st.color_space); }
	// sample i of a pass: its table entry, the capacity of its slot; the decoder behind the batch
	int entry_of(int i) const { return groups ? ((i & 1) ? ngroups + (i >> 1) : (i >> 1)) : i; }
	size_t cap_of(int i) { return thumbs ? thumb_cap : (groups ? ((i & 1) ? (size_t)kFollowerCap : group_cap) : dec.entropy().slot_bytes()); }
	size_t slots_bytes() { return thumbs ? thumb_cap * (size_t)n : (groups ? (size_t)ngroups * (group_cap + kFollowerCap) : dec.entropy().slot_bytes() * (size_t)n); }
	void *stream() { return thumbs ? thumb_stream : (groups ? gdec.stream() : dec.stream()); }
	int wait_stream() { if (thumbs) { if (hipStreamSynchronize((hipStream_t)thumb_stream) != hipSuccess) { (void)hipGetLastError(); return -2; } return 0; } return groups ? gdec.wait() : dec.wait(); }
	int picture_pitch() const { return thumbs ? 4 * thumb_w : (groups ? gdec.picture_pitch() : dec.picture_pitch()); }
	int picture_rows() const { return thumbs ? thumb_h : (groups ? gdec.picture_rows() : dec.picture_rows()); }
	size_t picture_bytes() const { return thumbs ? (size_t)4 * thumb_w * thumb_h : (groups ? gdec.picture_bytes() : dec.picture_bytes()); }
	uint8_t *device_pictures() const { return thumbs ? d_thumbs : (groups ? gdec.device_pictures() : dec.device_pictures()); }
	int finish_frame(int i, void *out, int pitch) { return groups ? gdec.finish_frame(i, out, pitch) : dec.finish_frame(i, out, pitch); }
	int download_frame(int i, void *out, int pitch) { return groups ? gdec.download_frame(i, out, pitch) : dec.download_frame(i, out, pitch); }
	// (a Bayer plan counts photosite quads: the mosaic is twice as wide)
	int picture_width() const { if (thumbs) return thumb_w; const int full = groups ? gst.plan.width : (st.plan.encoded_format == ENC_BAYER ? 2 * st.plan.width : st.plan.width); return (groups ? gst.half : st.half) ? full / 2 : full; }
	~cfhd_amd_decode_batch()
	{
		(void)hipSetDevice(device);
		dec.release(); gdec.release();
		if (scope_stream) device_stream_release(scope_stream);
		dec_parse_tables_release(&parse);
		if (thumb_stream) device_stream_destroy(thumb_stream);
		for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
		void *dv[] = { d_blob, d_table, d_sizes, d_verdicts, d_slots, d_thumbs }; for (void *p : dv) if (p) (void)hipFree(p);
		void *hv[] = { h_blob, h_table, h_verdicts, h_thumbs }; for (void *p : hv) if (p) (void)hipHostFree(p);
		if (slow) (void)CFHD_CloseDecoder(slow);
	}
};

namespace {
int allocate(cfhd_amd_decode_batch *b)
{
	b->blob_cap = b->slots_bytes() + 32;                 // a pass's samples fit whatever their alignment; a registered span with wider gaps is packed like plain memory
	b->table_bytes = b->groups ? b->table_dst_at() + 12 * (size_t)b->n : 12 * (size_t)b->n + 4 * ((size_t)b->n + 1);
	if (b->groups || b->thumbs) HIPCHK(hipMalloc((void **)&b->d_slots, b->slots_bytes()));
	if (!b->thumbs) HIPCHK(hipMalloc((void **)&b->d_blob, b->blob_cap));      // (a thumbnail batch: by its first submit_host -- samples that lie in HBM never need it)
	HIPCHK(hipMalloc((void **)&b->d_table, b->table_bytes));
	HIPCHK(hipHostMalloc((void **)&b->h_table, b->table_bytes, hipHostMallocPortable));
	HIPCHK(hipMalloc((void **)&b->d_sizes, 4 * (size_t)b->n));
	HIPCHK(hipMalloc((void **)&b->d_verdicts, 8 * (size_t)b->n));
	HIPCHK(hipHostMalloc((void **)&b->h_verdicts, 8 * (size_t)b->n, hipHostMallocPortable));
	HIPCHK(hipMemset(b->d_sizes, 0, 4 * (size_t)b->n));
	HIPCHK(hipMemset(b->d_verdicts, 0, 8 * (size_t)b->n));
	for (hipEvent_t &e : b->ev) HIPCHK(hipEventCreate(&e));
	return 0;
}

// k_dec_deliver over pictures [first, first + count) of the batch's own buffer, queued on the batch's stream: into the caller's device memory, in the layout it asked for.
// (slow_mode: the RGB_AS_YUV_* mode of a run of pictures the handle decoded in wait; -1: the launch of a pass, whose pictures are judged by their verdict words)
int launch_deliver(cfhd_amd_decode_batch *b, int first, int count, int slow_mode = -1)
{
	if (dev::deliver_is_rgb_as_yuv(b->dev_out_layout)) {  // the RG48 pictures of RGB samples as the YU64 picture, packed or as planes (set_device_pictures checked the geometry the kernel assumes)
		const bool pass = slow_mode < 0;                   // (first = 0: the verdict words are indexed by the picture)
		dev::k_dec_deliver_rgb_as_yuv<<<dim3(dev::dec_deliver_pieces(b->picture_rows()), (unsigned)count), dev::DEC_DELIVER_THREADS, 0, (hipStream_t)b->stream()>>>(
			b->device_pictures() + b->picture_bytes() * (size_t)first, b->picture_bytes(), b->picture_rows(), b->picture_width(),
			b->dev_out + b->dev_out_stride * (size_t)first, b->dev_out_stride, b->dev_out_pitch, b->dev_out_layout, pass ? dev::deliver_rgb_as_yuv_mode(b->st.color_space) : slow_mode,
			pass ? b->d_verdicts : nullptr, pass ? b->d_verdicts + b->n : nullptr, b->clean_word());
		HIPCHK(hipGetLastError());
		return 0;
	}
	if (dev::deliver_is_rgb10(b->dev_out_layout)) {      // the DPX0 thumbnails as three planes R, G, B of the 10-bit values (set_device_pictures checked the geometry)
		dev::k_dec_deliver_rgb10<<<dim3(dev::dec_deliver_pieces(b->picture_rows()), (unsigned)count), dev::DEC_DELIVER_THREADS, 0, (hipStream_t)b->stream()>>>(
			b->device_pictures() + b->picture_bytes() * (size_t)first, b->picture_bytes(), b->picture_rows(), b->picture_width(),
			b->dev_out + b->dev_out_stride * (size_t)first, b->dev_out_stride, b->dev_out_pitch, b->dev_out_layout);
		HIPCHK(hipGetLastError());
		return 0;
	}
	if (dev::deliver_is_bayer(b->dev_out_layout)) {      // the BYR4 mosaics of a Bayer batch as four planes (set_device_pictures checked the geometry the kernel assumes)
		const int quad_rows = b->picture_rows() / 2;
		dev::k_dec_deliver_bayer<<<dim3(dev::dec_deliver_pieces(quad_rows), (unsigned)count), dev::DEC_DELIVER_THREADS, 0, (hipStream_t)b->stream()>>>(
			b->device_pictures() + b->picture_bytes() * (size_t)first, b->picture_bytes(), quad_rows, b->picture_width() / 2,
			b->dev_out + b->dev_out_stride * (size_t)first, b->dev_out_stride, b->dev_out_pitch, dev::deliver_bayer_element(b->dev_out_layout));
		HIPCHK(hipGetLastError());
		return 0;
	}
	if (dev::deliver_is_yuv422(b->dev_out_layout)) {     // packed 4:2:2 pictures as a luma plane and two chroma planes (set_device_pictures checked the geometry the kernel assumes)
		const int order = b->st.out_kind == PIX_YU64 ? dev::YUV422_YU64 : (b->st.out_kind == PIX_2VUY ? dev::YUV422_2VUY : dev::YUV422_YUY2);
		dev::k_dec_deliver_yuv422<<<dim3(dev::dec_deliver_pieces(b->picture_rows()), (unsigned)count), dev::DEC_DELIVER_THREADS, 0, (hipStream_t)b->stream()>>>(
			b->device_pictures() + b->picture_bytes() * (size_t)first, b->picture_bytes(), b->picture_rows(), b->picture_width(),
			b->dev_out + b->dev_out_stride * (size_t)first, b->dev_out_stride, b->dev_out_pitch, b->dev_out_layout, order);
		HIPCHK(hipGetLastError());
		return 0;
	}
	if (dev::deliver_is_rgba(b->dev_out_layout)) {       // b64a, BGRA, BGRa pictures as four planes R, G, B, A, top row first (set_device_pictures checked the geometry the kernel assumes)
		const int order = b->st.out_kind == PIX_B64A ? dev::RGBA_B64A : (b->st.out_kind == PIX_BGRA ? dev::RGBA_BGRA : dev::RGBA_BGRa);
		dev::k_dec_deliver_rgba<<<dim3(dev::dec_deliver_pieces(b->picture_rows()), (unsigned)count), dev::DEC_DELIVER_THREADS, 0, (hipStream_t)b->stream()>>>(
			b->device_pictures() + b->picture_bytes() * (size_t)first, b->picture_bytes(), b->picture_rows(), b->picture_width(),
			b->dev_out + b->dev_out_stride * (size_t)first, b->dev_out_stride, b->dev_out_pitch, b->dev_out_layout, order);
		HIPCHK(hipGetLastError());
		return 0;
	}
	dev::k_dec_deliver<<<dim3(dev::dec_deliver_pieces(b->picture_rows()), (unsigned)count), dev::DEC_DELIVER_THREADS, 0, (hipStream_t)b->stream()>>>(
		b->device_pictures() + b->picture_bytes() * (size_t)first, b->picture_bytes(), b->picture_pitch(), b->picture_rows(), b->picture_width(),
		b->dev_out + b->dev_out_stride * (size_t)first, b->dev_out_stride, b->dev_out_pitch, b->dev_out_layout);
	HIPCHK(hipGetLastError());
	return 0;
}
// ... behind k_dec_blank in a pass, between two events of its own (cfhd_amd_decode_batch_kernel_ms index 9)
int launch_pass_deliver(cfhd_amd_decode_batch *b)
{
	hipStream_t st = (hipStream_t)b->stream();
	HIPCHK(hipEventRecord(b->ev[4], st));
	if (launch_deliver(b, 0, b->count)) return -5;
	HIPCHK(hipEventRecord(b->ev[5], st));
	b->deliver_timed = true;
	return 0;
}

// The same for a batch of two-frame groups: blob + table_src()[entry_of(i)] is sample i.  The table covers every entry of the batch -- those behind the pass are
// empty --, the decoder the count / 2 groups of the pass.
int launch_group_pass(cfhd_amd_decode_batch *b, const uint8_t *blob)
{
	hipStream_t st = (hipStream_t)b->stream();
	const int n = b->n, ng = b->ngroups;
	for (int j = 0; j < n; j++) b->table_size()[j] = 0u;
	for (int i = 0; i < b->count; i++) b->table_size()[b->entry_of(i)] = b->sizes[i];
	uint32_t pieces = 0;
	for (int j = 0; j < n; j++) {
		const bool follower = j >= ng;
		b->table_dst()[j] = follower ? (size_t)ng * b->group_cap + (size_t)(j - ng) * cfhd_amd_decode_batch::kFollowerCap : (size_t)j * b->group_cap;
		b->table_cap()[j] = (uint32_t)(follower ? (size_t)cfhd_amd_decode_batch::kFollowerCap : b->group_cap);
		b->table_first()[j] = pieces; pieces += dev::dec_ingest_pieces(b->table_size()[j], b->table_cap()[j]);
	}
	b->table_first()[n] = pieces;
	HIPCHK(hipMemcpyAsync(b->d_table, b->h_table, b->table_bytes, hipMemcpyHostToDevice, st));
	b->gdec.set_active(b->count / 2);
	HIPCHK(hipEventRecord(b->ev[0], st));
	dev::k_dec_ingest<<<pieces ? pieces : 1u, dev::DEC_INGEST_THREADS, 0, st>>>(blob, b->device_table(), n, b->d_slots, b->group_cap, b->d_sizes, b->d_verdicts + n);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(b->ev[1], st));
	// (the dither seed of pass k: as the intra batches')
	if (b->gdec.batch_entropy().launch() || b->gdec.launch_inverse(0xA511E9B3u * (b->steps + 1), true)) return -5;
	HIPCHK(hipEventRecord(b->ev[2], st));
	dev::k_dec_blank<<<dim3(dev::DEC_BLANK_SPLIT, (unsigned)b->count), dev::DEC_BLANK_THREADS, 0, st>>>(b->d_verdicts, b->d_verdicts + n, b->clean_word(), b->gdec.device_pictures(), b->gdec.picture_bytes(),
	                                                                                                      b->gdec.picture_pitch(), b->gdec.picture_pitch(), b->gdec.picture_rows(), ng);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(b->ev[3], st));
	b->timed = true;
	if (b->dev_out && launch_pass_deliver(b)) return -5;
	HIPCHK(hipMemcpyAsync(b->h_verdicts, b->d_verdicts, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
	if (b->host_out && b->gdec.download_frames(b->host_out, b->host_out_stride, b->host_out_pitch)) return -5;
	return 0;
}

// The same for a batch of thumbnails: k_dec_ingest, k_dec_parse, k_dec_thumbnail -- which writes the picture or the zeros of every sample of the pass --, the delivery.
int launch_thumbnail_pass(cfhd_amd_decode_batch *b, const uint8_t *blob)
{
	hipStream_t st = (hipStream_t)b->stream();
	const size_t cap = b->thumb_cap, picture_bytes = b->picture_bytes();
	uint32_t pieces = 0;
	for (int i = 0; i < b->count; i++) { b->table_size()[i] = b->sizes[i]; b->table_first()[i] = pieces; pieces += dev::dec_ingest_pieces(b->sizes[i], cap); }
	b->table_first()[b->count] = pieces;
	HIPCHK(hipMemcpyAsync(b->d_table, b->h_table, b->table_bytes, hipMemcpyHostToDevice, st));
	HIPCHK(hipEventRecord(b->ev[0], st));
	dev::k_dec_ingest<<<pieces ? pieces : 1u, dev::DEC_INGEST_THREADS, 0, st>>>(blob, b->device_table(), b->count, b->d_slots, cap, b->d_sizes, b->d_verdicts + b->n);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(b->ev[1], st));
	if (dec_parse_launch(b->parse, b->d_slots, cap, b->d_sizes, b->count, b->d_verdicts, st)) return -5;
	HIPCHK(hipEventRecord(b->ev[2], st));
	dev::k_dec_thumbnail<<<dim3(dev::dec_thumbnail_pieces(b->thumb_w * b->thumb_h), (unsigned)b->count), dev::DEC_THUMB_THREADS, 0, st>>>(
		(const dev::DecLowpassJob *)b->parse.d_lowjobs, b->parse.nch, b->d_verdicts, b->d_verdicts + b->n, b->thumb_w, b->thumb_h, b->thumb_yuv422, b->d_thumbs, picture_bytes);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(b->ev[3], st));
	b->timed = true;
	if (b->dev_out && launch_pass_deliver(b)) return -5;
	HIPCHK(hipMemcpyAsync(b->h_verdicts, b->d_verdicts, 8 * (size_t)b->n, hipMemcpyDeviceToHost, st));
	if (b->host_out) {
		// contiguous pictures in registered memory: one DMA into them; anything else through the batch's pinned memory, wait copies the rows out
		const size_t total = picture_bytes * (size_t)b->count;
		b->thumbs_staged = !(b->host_out_pitch == b->picture_pitch() && b->host_out_stride == picture_bytes && host_buffer_is_registered(b->host_out, total));
		if (b->thumbs_staged && !b->h_thumbs && hipHostMalloc((void **)&b->h_thumbs, picture_bytes * (size_t)b->n, hipHostMallocPortable) != hipSuccess) {
			(void)hipGetLastError(); b->h_thumbs = nullptr; device_set_last_error("decode queue: no pinned memory to stage the thumbnails"); return -5;
		}
		HIPCHK(hipMemcpyAsync(b->thumbs_staged ? b->h_thumbs : b->host_out, b->d_thumbs, total, hipMemcpyDeviceToHost, st));
	}
	return 0;
}

// Everything of a pass behind the samples' arrival in HBM, queued on the batch's stream: blob + table_src()[i] is sample i.  No host wait.
int launch_pass(cfhd_amd_decode_batch *b, const uint8_t *blob)
{
	(void)hipSetDevice(b->device);
	hipStream_t st = (hipStream_t)b->stream();
	if (b->groups) return launch_group_pass(b, blob);
	if (b->thumbs) return launch_thumbnail_pass(b, blob);
	const size_t cap = b->dec.entropy().slot_bytes();
	uint32_t pieces = 0;
	for (int i = 0; i < b->count; i++) { b->table_size()[i] = b->sizes[i]; b->table_first()[i] = pieces; pieces += dev::dec_ingest_pieces(b->sizes[i], cap); }
	b->table_first()[b->count] = pieces;
	HIPCHK(hipMemcpyAsync(b->d_table, b->h_table, b->table_bytes, hipMemcpyHostToDevice, st));
	b->dec.set_active(b->count);
	HIPCHK(hipEventRecord(b->ev[0], st));
	dev::k_dec_ingest<<<pieces ? pieces : 1u, dev::DEC_INGEST_THREADS, 0, st>>>(blob, b->device_table(), b->count, b->dec.entropy().sample_slots(), cap, b->d_sizes, b->d_verdicts + b->n);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(b->ev[1], st));
	// 8-bit outputs: the dither seed follows the pass number as the round-trip batch's does (cfhd_batch.cpp batch_launch): 0xA511E9B3 * (passes completed + 1)
	if (b->dec.launch_entropy() || b->dec.launch_inverse(0xA511E9B3u * (b->steps + 1))) return -5;
	HIPCHK(hipEventRecord(b->ev[2], st));
	dev::k_dec_blank<<<dim3(dev::DEC_BLANK_SPLIT, (unsigned)b->count), dev::DEC_BLANK_THREADS, 0, st>>>(b->d_verdicts, b->d_verdicts + b->n, b->clean_word(), b->dec.device_pictures(), b->dec.picture_bytes(),
	                                                                                                      b->dec.picture_pitch(), b->dec.picture_pitch(), b->dec.picture_rows());
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(b->ev[3], st));
	b->timed = true;
	if (b->dev_out && launch_pass_deliver(b)) return -5;
	HIPCHK(hipMemcpyAsync(b->h_verdicts, b->d_verdicts, 8 * (size_t)b->n, hipMemcpyDeviceToHost, st));
	if (b->host_out && b->dec.download_frames(b->host_out, b->host_out_stride, b->host_out_pitch)) return -5;
	return 0;
}

void begin_pass(cfhd_amd_decode_batch *b, const size_t *offsets, const size_t *sizes, int count)
{
	b->count = count;
	b->offsets.assign(offsets, offsets + count); b->full_sizes.assign(sizes, sizes + count);
	b->sizes.resize((size_t)count);
	for (int i = 0; i < count; i++) b->sizes[i] = sizes[i] > 0xfffffffeu ? 0xffffffffu : (uint32_t)sizes[i];
	// in front of the pass's first launch: the pass counts among the device's passes in flight until end_pass -- collected, or failed in submit
	if (!b->counted) { device_pass_begin(b->device); b->counted = true; b->dec.entropy().set_pass_counted(true); }
}
void end_pass(cfhd_amd_decode_batch *b)
{
	if (b->counted) { device_pass_end(b->device); b->counted = false; b->dec.entropy().set_pass_counted(false); }
	b->in_flight = false; b->src_host = b->src_device = nullptr; b->host_out = nullptr;
}
bool refuse(const char *text) { device_set_last_error(text); return false; }

// A batch of intra samples: cfhd_amd_decode_batch_create's, and -- bayer -- cfhd_amd_decode_batch_create_bayer's (the same gates and the same pass; the Bayer batch
// answers the mosaic's geometry and lets large launches take the fused last level, DecodeBatch::set_bayer_strips).
cfhd_amd_decode_batch *create_intra_batch(const void *first_sample, size_t first_size, uint32_t output_format, int decoded_resolution, int nsamples, bool bayer)
{
	if (!first_sample || first_size < 4) { refuse("decode queue: no first sample"); return nullptr; }
	if (nsamples < 1) { refuse("decode queue: nsamples < 1"); return nullptr; }
	{ const char *e = getenv("CFHD_AMD_ENTROPY"); if (e && strcmp(e, "host") == 0) { refuse("decode queue: CFHD_AMD_ENTROPY=host keeps the entropy stage on the host (the C ABI's arrangement)"); return nullptr; } }
	const uint8_t *s8 = (const uint8_t *)first_sample;
	const int first_tag = (int16_t)((s8[0] << 8) | s8[1]), sample_type = (s8[2] << 8) | s8[3];
	if (first_tag == TAG_SAMPLE && (sample_type == 7 || sample_type == 2 || sample_type == 1)) { refuse("decode queue: two-frame groups (group samples, P-frame samples, sequence headers) are decoded by cfhd_amd_decode_batch_create_groups or CFHD_DecodeSample"); return nullptr; }
	ParsedSample ps;
	const int parsed = parse_sample(s8, first_size, &ps);
	const bool uncompressed = ps.uncompressed;           // (an UNCOMPRESS chunk: CFHD_PrepareToDecode refuses below with its own text)
	if (!bayer && parsed >= 0 && ps.encoded_format == ENC_BAYER) { refuse("decode queue: Bayer samples are decoded by CFHD_DecodeSample"); return nullptr; }
	if (bayer) {
		// served for what the handle serves: the BYR4 mosaic at full resolution (decoded_resolution 0 is taken as full, as CFHD_PrepareToDecode takes it)
		if (!uncompressed && (parsed < 0 || ps.encoded_format != ENC_BAYER)) { refuse("decode queue: a Bayer batch is prepared on a Bayer intra sample; other intra samples go to cfhd_amd_decode_batch_create"); return nullptr; }
		if (output_format != 0x42595234u /* 'BYR4' */) { refuse("decode queue: Bayer samples decode to BYR4, the raw mosaic (no other output is built)"); return nullptr; }
		if (decoded_resolution != 0 && decoded_resolution != 1) { refuse("decode queue: Bayer samples decode at full resolution only"); return nullptr; }
	}
	cfhd_amd_decode_batch *b = new (std::nothrow) cfhd_amd_decode_batch;
	if (!b) return nullptr;
	b->n = nsamples;
	auto fail = [&](const char *text) { if (text) device_set_last_error(text); delete b; return (cfhd_amd_decode_batch *)nullptr; };
	// the handle's gates: CFHD_PrepareToDecode on the whole first sample, then that sample through CFHD_DecodeSample once (the scan is only known there)
	char text[200];
	if (CFHD_OpenDecoder(&b->slow, nullptr) != ERR_OKAY) return fail("decode queue: no decoder handle");
	int aw = 0, ah = 0; CFHD_PixelFormat af = 0; int32_t pitch = 0;
	int rc = CFHD_PrepareToDecode(b->slow, 0, 0, output_format, decoded_resolution, 0, (void *)first_sample, first_size, &aw, &ah, &af);
	if (rc != ERR_OKAY) {
		if (!uncompressed) { snprintf(text, sizeof(text), "decode queue: CFHD_PrepareToDecode refuses this sample, output and resolution (CFHD_Error %d)", rc); return fail(text); }
		return fail(nullptr);                              // (the uncompressed mode: the handle's own text)
	}
	if (CFHD_GetImagePitch((uint32_t)aw, af, &pitch) != ERR_OKAY || pitch <= 0 || ah <= 0) return fail("decode queue: no picture geometry");
	{
		std::vector<uint8_t> scratch((size_t)pitch * ah);
		device_set_last_error("");
		rc = CFHD_DecodeSample(b->slow, (void *)first_sample, first_size, scratch.data(), pitch);
		if (rc != ERR_OKAY) {
			if (*device_last_error()) return fail(nullptr);      // (the device layer said why: output_route()'s refusal texts, a missing device)
			snprintf(text, sizeof(text), "decode queue: CFHD_DecodeSample refuses this sample, output and resolution (CFHD_Error %d)", rc); return fail(text);
		}
	}
	if (decoder_handle_state(b->slow, &b->st)) return fail("decode queue: the first sample is not an intra sample");
	// (k_dec_lowpass and the plane transforms carry sample x channel in a grid dimension)
	if ((long long)nsamples * b->st.plan.num_channels > 65535) return fail("decode queue: the batch's job index would pass the grid limit (65 535)");
	// on the calling thread's device, one stream for the whole pass, as cfhd_amd_batch_create_ex places its batches
	struct Lean { Lean() { device_streams_lean(true); } ~Lean() { device_streams_lean(false); } } lean;
	{
		StreamScope scope;
		b->dec.set_interlaced(b->st.interlaced);
		b->dec.set_bayer_strips(bayer);
		const int prc = b->dec.prepare(b->st.plan, nsamples, b->st.out_kind, b->st.half) || b->dec.prepare_entropy(b->st.sample_cap);
		b->scope_stream = scope.stream();
		if (prc) return fail(nullptr);
	}
	b->device = device_current();
	if (!b->dec.entropy().chunk_indexed()) return fail("decode queue: the chunk-indexed band decoder only (CFHD_AMD_DEC is set)");
	if (allocate(b)) return fail("decode queue: out of device or pinned memory");
	if (b->dec.entropy().set_samples_device(b->dec.entropy().sample_slots(), b->dec.entropy().slot_bytes(), b->d_sizes)) return fail("decode queue: sample slots");
	b->dec.entropy().set_verdicts(b->d_verdicts);
	b->slow_pictures.resize((size_t)nsamples);
	return b;
}
}

extern "C" {

cfhd_amd_decode_batch *cfhd_amd_decode_batch_create(const void *first_sample, size_t first_size, uint32_t output_format, int decoded_resolution, int nsamples)
{
	CallerDevice caller_device;
	return create_intra_batch(first_sample, first_size, output_format, decoded_resolution, nsamples, false);
}

// Bayer intra samples to BYR4 (include/cfhd_amd.h): cfhd_amd_decode_batch_create's batch with the mosaic as the picture; every other entry point is shared.
cfhd_amd_decode_batch *cfhd_amd_decode_batch_create_bayer(const void *first_sample, size_t first_size, uint32_t output_format, int decoded_resolution, int nsamples)
{
	CallerDevice caller_device;
	return create_intra_batch(first_sample, first_size, output_format, decoded_resolution, nsamples, true);
}

cfhd_amd_decode_batch *cfhd_amd_decode_batch_create_groups(const void *first_group_sample, size_t first_size, uint32_t output_format, int decoded_resolution, int ngroups)
{
	CallerDevice caller_device;
	if (!first_group_sample || first_size < 4) { refuse("decode queue: no first group sample"); return nullptr; }
	if (ngroups < 1) { refuse("decode queue: ngroups < 1"); return nullptr; }
	{ const char *e = getenv("CFHD_AMD_ENTROPY"); if (e && strcmp(e, "host") == 0) { refuse("decode queue: CFHD_AMD_ENTROPY=host keeps the entropy stage on the host (the C ABI's arrangement)"); return nullptr; } }
	const uint8_t *s8 = (const uint8_t *)first_group_sample;
	const int first_tag = (int16_t)((s8[0] << 8) | s8[1]), sample_type = (s8[2] << 8) | s8[3];
	if (first_tag != TAG_SAMPLE || sample_type != 2) {
		refuse(first_tag == TAG_SAMPLE && sample_type == 7 ? "decode queue: a batch of groups is prepared on a group sample, not on the sequence header (a reader skips it)"
		       : first_tag == TAG_SAMPLE && sample_type == 1 ? "decode queue: a batch of groups is prepared on a group sample, not on the P-frame sample behind one"
		       : "decode queue: a batch of groups is prepared on a group sample; intra samples go to cfhd_amd_decode_batch_create");
		return nullptr;
	}
	// (k_dec_lowpass and the plane transforms carry group x 6 jobs in a grid dimension: GpuGroupBatchEntropyDecoder::prepare, GopBatch::prepare)
	if (6LL * ngroups > 65535) { refuse("decode queue: the batch's job index would pass the grid limit (65 535)"); return nullptr; }
	cfhd_amd_decode_batch *b = new (std::nothrow) cfhd_amd_decode_batch;
	if (!b) return nullptr;
	b->groups = true; b->ngroups = ngroups; b->n = 2 * ngroups;
	auto fail = [&](const char *text) { if (text) device_set_last_error(text); delete b; return (cfhd_amd_decode_batch *)nullptr; };
	// the handle's gates, as cfhd_amd_decode_batch_create: CFHD_PrepareToDecode on the group sample, then that sample through CFHD_DecodeSample once (the scan is only known there)
	char text[200];
	if (CFHD_OpenDecoder(&b->slow, nullptr) != ERR_OKAY) return fail("decode queue: no decoder handle");
	int aw = 0, ah = 0; CFHD_PixelFormat af = 0; int32_t pitch = 0;
	int rc = CFHD_PrepareToDecode(b->slow, 0, 0, output_format, decoded_resolution, 0, (void *)first_group_sample, first_size, &aw, &ah, &af);
	if (rc != ERR_OKAY) { snprintf(text, sizeof(text), "decode queue: CFHD_PrepareToDecode refuses this sample, output and resolution (CFHD_Error %d)", rc); return fail(text); }
	if (CFHD_GetImagePitch((uint32_t)aw, af, &pitch) != ERR_OKAY || pitch <= 0 || ah <= 0) return fail("decode queue: no picture geometry");
	{
		std::vector<uint8_t> scratch((size_t)pitch * ah);
		device_set_last_error("");
		rc = CFHD_DecodeSample(b->slow, (void *)first_group_sample, first_size, scratch.data(), pitch);
		if (rc != ERR_OKAY) {
			if (*device_last_error()) return fail(nullptr);      // (the device layer said why)
			snprintf(text, sizeof(text), "decode queue: CFHD_DecodeSample refuses this sample, output and resolution (CFHD_Error %d)", rc); return fail(text);
		}
	}
	if (decoder_group_state(b->slow, &b->gst)) return fail("decode queue: the first sample is not a group sample");
	{
		// what the verdict of a clean group of the prepared kind carries, and the matrix of the outputs that convert to RGB (decode_group_sample)
		ParsedGroup pg;
		if (parse_group_sample(s8, first_size, &pg) != 0) return fail("decode queue: the first sample is not a group sample");
		b->st.progressive_flag = pg.progressive != 0; b->st.color_space = pg.color_space; b->st.interlaced = b->gst.plan.interlaced; b->st.half = b->gst.half; b->st.out_kind = b->gst.out_kind;
	}
	const GopPlan &gp = b->gst.plan;
	b->group_cap = ((size_t)gp.width * gp.display_height * 8 + 131072 + 255) & ~(size_t)255;      // the handle's (decode_group_sample)
	struct Lean { Lean() { device_streams_lean(true); } ~Lean() { device_streams_lean(false); } } lean;
	{
		StreamScope scope;
		int prc = b->gdec.prepare(gp, true, b->gst.out_kind, b->gst.half, ngroups);
		b->scope_stream = scope.stream();
		if (prc) return fail(nullptr);
		prc = b->gdec.prepare_entropy_decode();
		if (prc < 0) return fail("decode queue: the device stage does not take groups of this geometry (CFHD_DecodeSample decodes them)");
		if (prc) return fail("decode queue: out of device or pinned memory");
	}
	b->device = device_current();
	b->gdec.set_color_matrix((b->st.color_space & 3) == 1 ? 2 : 0);
	b->gdec.set_timed(true);
	if (allocate(b)) return fail("decode queue: out of device or pinned memory");
	GpuGroupBatchEntropyDecoder &ent = b->gdec.batch_entropy();
	if (ent.set_samples_slots(b->d_slots, b->group_cap, b->d_sizes, b->d_slots + (size_t)ngroups * b->group_cap, cfhd_amd_decode_batch::kFollowerCap, b->d_sizes + ngroups)) return fail("decode queue: sample slots");
	ent.set_verdicts(b->d_verdicts);
	snprintf(b->band_name, sizeof(b->band_name), "%s%s+k_dec_band_two_pass", ent.band_kernel(), gp.interlaced ? "+k_dec_undiff" : "");
	b->slow_pictures.resize((size_t)b->n);
	return b;
}

// Thumbnails of a batch of intra samples (include/cfhd_amd.h): the front of the decode pass -- k_dec_ingest, k_dec_parse -- and k_dec_thumbnail on the raw lowpass words;
// every other entry point is shared.  The gates are CFHD_GetThumbnail's on the first sample, the geometry its answer.
cfhd_amd_decode_batch *cfhd_amd_decode_batch_create_thumbnails(const void *first_sample, size_t first_size, int nsamples)
{
	CallerDevice caller_device;
	if (!first_sample || first_size < 4) { refuse("decode queue: no first sample"); return nullptr; }
	if (nsamples < 1) { refuse("decode queue: nsamples < 1"); return nullptr; }
	if (nsamples > 65535) { refuse("decode queue: a thumbnail batch carries its pictures in a grid dimension: nsamples <= 65 535"); return nullptr; }
	{ const char *e = getenv("CFHD_AMD_ENTROPY"); if (e && strcmp(e, "host") == 0) { refuse("decode queue: CFHD_AMD_ENTROPY=host keeps the entropy stage on the host (the C ABI's arrangement)"); return nullptr; } }
	const uint8_t *s8 = (const uint8_t *)first_sample;
	const int first_tag = (int16_t)((s8[0] << 8) | s8[1]), sample_type = (s8[2] << 8) | s8[3];
	if (first_tag == TAG_SAMPLE && (sample_type == 7 || sample_type == 2 || sample_type == 1)) {
		refuse("decode queue: thumbnails of two-frame groups (group samples, P-frame samples, sequence headers) are not built; CFHD_GetThumbnail serves intra samples"); return nullptr;
	}
	ParsedSample ps;
	const int parsed = parse_sample(s8, first_size, &ps);
	if (ps.uncompressed) { refuse("decode queue: a sample of the uncompressed mode (an UNCOMPRESS chunk) has no lowpass bands to make a thumbnail of"); return nullptr; }
	if (parsed >= 0 && ps.encoded_format == ENC_BAYER) { refuse("decode queue: Bayer thumbnails are not built (the reference makes them by a quarter-resolution decode; CFHD_GetThumbnail answers CFHD_ERROR_BADFORMAT)"); return nullptr; }
	const size_t w8 = parsed == 0 ? (size_t)(ps.width + 7) / 8 : 0, h8 = parsed == 0 ? (size_t)(ps.height + 7) / 8 : 0;
	char text[200];
	if (w8 & 1) { snprintf(text, sizeof(text), "decode queue: the thumbnail of this sample is %d pixels wide: CFHD_GetThumbnail writes even widths only", (int)w8); refuse(text); return nullptr; }
	cfhd_amd_decode_batch *b = new (std::nothrow) cfhd_amd_decode_batch;
	if (!b) return nullptr;
	b->n = nsamples; b->thumbs = true;
	auto fail = [&](const char *t) { if (t) device_set_last_error(t); delete b; return (cfhd_amd_decode_batch *)nullptr; };
	if (CFHD_OpenDecoder(&b->slow, nullptr) != ERR_OKAY) return fail("decode queue: no decoder handle");
	{
		// CFHD_GetThumbnail's own verdict on the first sample (it checks the lowpass bands against the sample's size before it looks at the buffer)
		std::vector<uint8_t> scratch(w8 * h8 * 6 <= first_size && w8 * h8 ? w8 * h8 * 4 : 16);
		size_t rw = 0, rh = 0, rsize = 0;
		const int rc = CFHD_GetThumbnail(b->slow, (void *)first_sample, first_size, scratch.data(), scratch.size(), 0, &rw, &rh, &rsize);
		if (rc != ERR_OKAY || rw != w8 || rh != h8) { snprintf(text, sizeof(text), "decode queue: CFHD_GetThumbnail refuses this sample (CFHD_Error %d)", rc); return fail(text); }
	}
	// what k_dec_parse checks a sample against: the plan of the sample's geometry (any output of it: no picture is decoded); its lowpass bands are the thumbnail's
	FramePlan plan;
	if (!build_frame_plan(&plan, ps.width, ps.display_height ? ps.display_height : ps.height, PIX_RG48, ps.encoded_format)) return fail("decode queue: a geometry the device parser does not take (CFHD_GetThumbnail serves it)");
	const bool yuv422 = ps.encoded_format == ENC_YUV422;
	for (int c = 0; c < 3; c++) {
		const BandDesc &ll = plan.ch[c].band[2][0];
		if (ll.width != (int)(yuv422 && c ? w8 / 2 : w8) || ll.height != (int)h8) return fail("decode queue: a geometry the device parser does not take (CFHD_GetThumbnail serves it)");
	}
	b->thumb_w = (int)w8; b->thumb_h = (int)h8; b->thumb_yuv422 = yuv422;
	// a slot holds what the handles' device stage takes of such a sample: width x height x bytes per pixel of its 16-bit picture + 64 KB
	b->thumb_cap = ((size_t)plan.width * plan.height * (yuv422 ? 2 : (ps.encoded_format == ENC_RGB444 ? 6 : 8)) + 65536 + 255) & ~(size_t)255;
	if (device_init()) return fail(nullptr);
	b->device = device_current();
	(void)hipSetDevice(b->device);
	if (device_stream_create(&b->thumb_stream)) return fail("decode queue: no stream");
	if (allocate(b) || dec_parse_tables_prepare(plan, nsamples, &b->parse) || hipMalloc((void **)&b->d_thumbs, b->picture_bytes() * (size_t)nsamples) != hipSuccess ||
	    hipMemset(b->d_thumbs, 0, b->picture_bytes() * (size_t)nsamples) != hipSuccess) { (void)hipGetLastError(); return fail("decode queue: out of device or pinned memory"); }
	b->slow_pictures.resize((size_t)nsamples);
	return b;
}

void cfhd_amd_decode_batch_destroy(cfhd_amd_decode_batch *b)
{
	CallerDevice caller_device;
	if (b && b->in_flight) (void)cfhd_amd_decode_batch_wait(b, nullptr);
	delete b;
}

int cfhd_amd_decode_batch_geometry(cfhd_amd_decode_batch *b, int *width, int *height, int *row_bytes)
{
	if (!b || b->in_flight) return -1;
	if (width) *width = b->picture_width();
	if (height) *height = b->picture_rows();
	if (row_bytes) *row_bytes = b->picture_pitch();
	return 0;
}

int cfhd_amd_decode_batch_set_device_pictures(cfhd_amd_decode_batch *b, void *d_pictures, size_t picture_stride, int picture_pitch, int layout)
{
	if (!b) { refuse("decode queue: no batch"); return -1; }
	if (b->in_flight) { refuse("decode queue: device pictures are set between passes, not while one is in flight"); return -1; }
	if (!d_pictures) { b->dev_out = nullptr; return 0; }
	if (b->thumbs && layout != CFHD_AMD_PICTURES_PACKED) {
		// (the RGB10_* layouts exist for the DPX0 words of a thumbnail batch alone: to every other batch they are unknown, below)
		if (layout >= CFHD_AMD_PICTURES_PLANAR_U16 && layout <= CFHD_AMD_PICTURES_RGB_AS_YUV422_F32) {
			refuse("decode queue: a thumbnail batch delivers its DPX0 words (CFHD_AMD_PICTURES_PACKED) or the planes R, G, B of their 10-bit values (CFHD_AMD_PICTURES_RGB10_U16 / _F16 / _F32)"); return -1;
		}
		if (!dev::deliver_is_rgb10(layout)) { refuse("decode queue: unknown layout of the device pictures"); return -1; }
		if (((uintptr_t)d_pictures | picture_stride | (size_t)(unsigned)picture_pitch) & 15) { refuse("decode queue: the device pictures' pointer, stride and pitch are multiples of 16"); return -1; }
		// three planes of H rows at the pitch, of which the last row needs its row bytes only
		const long long plane_row = (long long)b->thumb_w * dev::deliver_rgb10_element_bytes(layout);
		if (picture_pitch < plane_row) { refuse("decode queue: the pitch is below the plane row of the RGB10 layout (width x element size)"); return -1; }
		if (picture_stride < (size_t)picture_pitch * (3 * (size_t)b->thumb_h - 1) + (size_t)plane_row) { refuse("decode queue: the stride is below the three planes of the RGB10 layout (3 x H rows a pitch apart)"); return -1; }
		b->dev_out = (uint8_t *)d_pictures; b->dev_out_stride = picture_stride; b->dev_out_pitch = picture_pitch; b->dev_out_layout = layout;
		return 0;
	}
	// (the BAYER_* layouts exist for the BYR4 mosaics of cfhd_amd_decode_batch_create_bayer's batches alone: to every other batch they are unknown)
	const bool bayer = dev::deliver_is_bayer(layout) && !b->groups && b->st.out_kind == PIX_BYR4;
	// (the YUV422_* layouts exist for packed 4:2:2 pictures: to a Bayer batch they are unknown, every other output that is not YUY2, 2vuy or YU64 is told so)
	const bool yuv422 = dev::deliver_is_yuv422(layout) && b->st.out_kind != PIX_BYR4;
	// (the RGBA_* layouts exist for the pictures that carry an alpha component -- b64a, BGRA, BGRa --: to every other batch they are unknown)
	const bool rgba = dev::deliver_is_rgba(layout) && (b->st.out_kind == PIX_B64A || b->st.out_kind == PIX_BGRA || b->st.out_kind == PIX_BGRa);
	// (the RGB_AS_* layouts exist for RG48 pictures: to every batch with another output they are unknown)
	const bool rgb_as_yuv = dev::deliver_is_rgb_as_yuv(layout) && b->st.out_kind == PIX_RG48;
	if (!bayer && !yuv422 && !rgba && !rgb_as_yuv && (layout < CFHD_AMD_PICTURES_PACKED || layout > CFHD_AMD_PICTURES_PLANAR_F32)) { refuse("decode queue: unknown layout of the device pictures"); return -1; }
	if (yuv422) {
		const int kind = b->st.out_kind;
		if (kind != PIX_YUY2 && kind != PIX_2VUY && kind != PIX_YU64) { refuse("decode queue: the 4:2:2 plane layouts serve batches whose output is YUY2, 2vuy or YU64"); return -1; }
		if (layout == CFHD_AMD_PICTURES_YUV422_U8 && kind == PIX_YU64) { refuse("decode queue: YUV422_U8 serves the 8-bit outputs YUY2 and 2vuy; a YU64 batch delivers YUV422_U16"); return -1; }
		if (layout == CFHD_AMD_PICTURES_YUV422_U16 && kind != PIX_YU64) { refuse("decode queue: YUV422_U16 serves YU64; a YUY2 or 2vuy batch delivers YUV422_U8"); return -1; }
	}
	if (rgba) {
		if (layout == CFHD_AMD_PICTURES_RGBA_U8 && b->st.out_kind == PIX_B64A) { refuse("decode queue: RGBA_U8 serves the 8-bit outputs BGRA and BGRa; a b64a batch delivers RGBA_U16"); return -1; }
		if (layout == CFHD_AMD_PICTURES_RGBA_U16 && b->st.out_kind != PIX_B64A) { refuse("decode queue: RGBA_U16 serves b64a; a BGRA or BGRa batch delivers RGBA_U8"); return -1; }
	}
	if (rgb_as_yuv) {
		const int enc = b->st.plan.encoded_format;
		if (b->groups || b->st.half || (enc != ENC_RGB444 && enc != ENC_RGBA4444)) {
			refuse("decode queue: the RGB_AS_* layouts serve full-resolution RG48 batches of RGB 4:4:4 and RGBA 4:4:4:4 samples (the YU64 picture of the RG48 one); a 4:2:2 sample decodes to YU64 directly"); return -1;
		}
		if (b->picture_width() & 1) { refuse("decode queue: the RGB_AS_* layouts pair the pixels of a row: the width is even"); return -1; }
	}
	const bool planar = !bayer && !yuv422 && !rgba && !rgb_as_yuv && layout != CFHD_AMD_PICTURES_PACKED;
	if (planar && b->st.out_kind != PIX_RG48) { refuse("decode queue: the planar layouts serve batches whose output is RG48"); return -1; }
	if (((uintptr_t)d_pictures | picture_stride | (size_t)(unsigned)picture_pitch) & 15) { refuse("decode queue: the device pictures' pointer, stride and pitch are multiples of 16"); return -1; }
	if (yuv422) {
		// Y at the pitch, Cb and Cr at half of it: H * pitch + 2 H * (pitch / 2) bytes a picture, of which the last chroma row needs its row bytes only
		if (picture_pitch & 31) { refuse("decode queue: the pitch of a 4:2:2 plane layout is a multiple of 32 (the chroma planes' is half of it)"); return -1; }
		const int w = b->picture_width(), h = b->picture_rows(), word = b->st.out_kind == PIX_YU64 ? 2 : 1;
		const long long luma_row = (long long)w * dev::deliver_yuv422_element_bytes(layout);
		// what k_dec_deliver_yuv422 assumes of the batch's own pictures: whole groups of eight pixels, rows back to back on 16-byte boundaries
		if ((w & 7) || b->picture_pitch() != 2 * word * w || b->picture_bytes() != (size_t)b->picture_pitch() * (size_t)h || ((uintptr_t)b->device_pictures() & 15) || b->n > 65535 /* blockIdx.y */) {
			refuse("decode queue: pictures the 4:2:2 deliver kernel does not take"); return -1;
		}
		if (picture_pitch < luma_row) { refuse("decode queue: the pitch is below the luma row of the 4:2:2 plane layout (width x element size)"); return -1; }
		if (picture_stride < (size_t)picture_pitch * (size_t)h + (size_t)(picture_pitch / 2) * (2 * (size_t)h - 1) + (size_t)(luma_row / 2)) {
			refuse("decode queue: the stride is below the three planes of the 4:2:2 layout (H x pitch, then 2 H chroma rows pitch / 2 apart)"); return -1;
		}
		b->dev_out = (uint8_t *)d_pictures; b->dev_out_stride = picture_stride; b->dev_out_pitch = picture_pitch; b->dev_out_layout = layout;
		return 0;
	}
	if (rgb_as_yuv) {
		const bool packed = layout == CFHD_AMD_PICTURES_RGB_AS_YU64;
		const int w = b->picture_width(), h = b->picture_rows();
		// what k_dec_deliver_rgb_as_yuv assumes of the batch's own pictures: rows of 6 x width bytes back to back, the pictures on 16-byte boundaries
		if (b->picture_pitch() != 6 * w || b->picture_bytes() != (size_t)b->picture_pitch() * (size_t)h || (((uintptr_t)b->device_pictures() | b->picture_bytes()) & 15) || b->n > 65535 /* blockIdx.y */) {
			refuse("decode queue: pictures the RGB-as-YUV deliver kernel does not take"); return -1;
		}
		if (packed) {
			// H rows of 4 x W bytes at the pitch, of which the last needs its row bytes only
			if (picture_pitch < 4LL * w) { refuse("decode queue: the pitch is below the row of the RGB_AS_YU64 layout (4 x width bytes)"); return -1; }
			if (picture_stride < (size_t)picture_pitch * (size_t)(h - 1) + 4 * (size_t)w) { refuse("decode queue: the stride is below the rows of the RGB_AS_YU64 layout (H rows a pitch apart)"); return -1; }
		} else {
			// the geometry of the YUV422_* layouts: Y at the pitch, Cb and Cr at half of it
			if (picture_pitch & 31) { refuse("decode queue: the pitch of an RGB_AS_YUV422 layout is a multiple of 32 (the chroma planes' is half of it)"); return -1; }
			const long long luma_row = (long long)w * dev::deliver_rgb_as_yuv_element_bytes(layout);
			if (picture_pitch < luma_row) { refuse("decode queue: the pitch is below the luma row of the RGB_AS_YUV422 layout (width x element size)"); return -1; }
			if (picture_stride < (size_t)picture_pitch * (size_t)h + (size_t)(picture_pitch / 2) * (2 * (size_t)h - 1) + (size_t)(luma_row / 2)) {
				refuse("decode queue: the stride is below the three planes of the RGB_AS_YUV422 layout (H x pitch, then 2 H chroma rows pitch / 2 apart)"); return -1;
			}
		}
		b->dev_out = (uint8_t *)d_pictures; b->dev_out_stride = picture_stride; b->dev_out_pitch = picture_pitch; b->dev_out_layout = layout;
		return 0;
	}
	if (rgba) {
		// four planes of H rows at the pitch, of which the last row needs its row bytes only
		const int w = b->picture_width(), h = b->picture_rows(), pixel = b->st.out_kind == PIX_B64A ? 8 : 4;
		const long long plane_row = (long long)w * dev::deliver_rgba_element_bytes(layout);
		// what k_dec_deliver_rgba assumes of the batch's own pictures: rows of whole pixels back to back, the pictures on 16-byte boundaries (rows that are no multiple of
		// 16 bytes long go element by element: no width the queue serves has them)
		if (b->picture_pitch() != pixel * w || b->picture_bytes() != (size_t)b->picture_pitch() * (size_t)h || (((uintptr_t)b->device_pictures() | b->picture_bytes()) & 15) || b->n > 65535 /* blockIdx.y */) {
			refuse("decode queue: pictures the RGBA deliver kernel does not take"); return -1;
		}
		if (picture_pitch < plane_row) { refuse("decode queue: the pitch is below the plane row of the RGBA layout (width x element size)"); return -1; }
		if (picture_stride < (size_t)picture_pitch * (4 * (size_t)h - 1) + (size_t)plane_row) { refuse("decode queue: the stride is below the four planes of the RGBA layout (4 x H rows a pitch apart)"); return -1; }
		b->dev_out = (uint8_t *)d_pictures; b->dev_out_stride = picture_stride; b->dev_out_pitch = picture_pitch; b->dev_out_layout = layout;
		return 0;
	}
	// the rows and planes a picture has in the layout: the mosaic's four planes are half as high and half as wide
	const int rows = bayer ? b->picture_rows() / 2 : b->picture_rows(), planes = bayer ? 4 : (planar ? 3 : 1);
	const int elt = layout == CFHD_AMD_PICTURES_PLANAR_F32 || layout == CFHD_AMD_PICTURES_BAYER_F32 ? 4 : 2;
	const long long row_bytes = bayer ? (long long)(b->picture_width() / 2) * elt : (planar ? (long long)b->picture_width() * elt : b->picture_pitch());
	// what k_dec_deliver_bayer assumes of the batch's own pictures: whole quads, plane rows of whole groups of eight, mosaic rows back to back on 16-byte boundaries
	if (bayer && ((b->picture_width() & 15) || (b->picture_rows() & 1) || b->picture_pitch() != 2 * b->picture_width() || b->picture_bytes() != (size_t)b->picture_pitch() * (size_t)b->picture_rows() ||
	              ((uintptr_t)b->device_pictures() & 15) || b->n > 65535 /* blockIdx.y */)) { refuse("decode queue: mosaics the Bayer deliver kernel does not take"); return -1; }
	if (picture_pitch < row_bytes) { refuse("decode queue: the device pictures' pitch is below the row bytes of the layout"); return -1; }
	if (picture_stride < (size_t)picture_pitch * ((size_t)planes * rows - 1) + (size_t)row_bytes) { refuse("decode queue: the device pictures' stride is below what one picture occupies"); return -1; }
	b->dev_out = (uint8_t *)d_pictures; b->dev_out_stride = picture_stride; b->dev_out_pitch = picture_pitch; b->dev_out_layout = layout;
	return 0;
}

int cfhd_amd_decode_batch_submit_host(cfhd_amd_decode_batch *b, const void *base, const size_t *offsets, const size_t *sizes, int count, void *pictures, size_t picture_stride, int picture_pitch)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || !base || !offsets || !sizes || count < 1 || count > b->n || (b->groups && (count & 1))) return -1;
	if (pictures && (picture_pitch < b->picture_pitch() || picture_stride < (size_t)picture_pitch * (size_t)(b->picture_rows() - 1) + (size_t)b->picture_pitch())) return -1;
	(void)hipSetDevice(b->device);
	if (!b->d_blob && hipMalloc((void **)&b->d_blob, b->blob_cap) != hipSuccess) { (void)hipGetLastError(); b->d_blob = nullptr; device_set_last_error("decode queue: no device memory to stage the samples"); return -2; }      // (a thumbnail batch's first pass from host memory)
	begin_pass(b, offsets, sizes, count);
	const std::vector<uint32_t> &size = b->sizes;
	auto placed = [&](int i) { return dev::dec_ingest_pieces(size[i], b->cap_of(i)) != 0; };      // sample i is one k_dec_ingest copies
	size_t lo = ~(size_t)0, hi = 0;                        // the span of the samples k_dec_ingest will place
	for (int i = 0; i < count; i++)
		if (placed(i)) { if (offsets[i] < lo) lo = offsets[i]; if (offsets[i] + sizes[i] > hi) hi = offsets[i] + sizes[i]; }
	b->src_host = (const uint8_t *)base; b->src_device = nullptr;
	b->host_out = (uint8_t *)pictures; b->host_out_stride = picture_stride; b->host_out_pitch = picture_pitch;
	hipStream_t st = (hipStream_t)b->stream();
	int rc = 0;
	if (b->groups) for (int j = 0; j < b->n; j++) b->table_src()[j] = 0;      // (the entries behind a short pass)
	if (hi <= lo) {                                        // nothing to copy: every sample is empty or the slow path's
		for (int i = 0; i < count; i++) b->table_src()[b->entry_of(i)] = 0;
	} else if (hi - lo <= b->blob_cap - 32 && host_buffer_is_registered((const uint8_t *)base + lo, hi - lo)) {
		// a registered blob: one DMA of the span as it lies, k_dec_ingest aligns
		for (int i = 0; i < count; i++) b->table_src()[b->entry_of(i)] = placed(i) ? offsets[i] - lo : 0;
		if (hipMemcpyAsync(b->d_blob, (const uint8_t *)base + lo, hi - lo, hipMemcpyHostToDevice, st) != hipSuccess) rc = -2;
	} else {
		// plain memory (or a span with gaps wider than the batch's buffer): the calling thread packs the samples back to back into pinned memory -- the only host
		// work of a pass, in front of its first launch --, then the same DMA and the same kernel
		size_t at = 0;
		if (!b->h_blob && hipHostMalloc((void **)&b->h_blob, b->blob_cap, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); b->h_blob = nullptr; end_pass(b); device_set_last_error("decode queue: no pinned memory to stage the samples"); return -2; }
		for (int i = 0; i < count; i++) { b->table_src()[b->entry_of(i)] = at; if (placed(i)) at += size[i]; }
		parallel_for(count, count > 8 ? 8 : 1, [&](int i) { if (placed(i)) memcpy(b->h_blob + b->table_src()[b->entry_of(i)], (const uint8_t *)base + offsets[i], size[i]); });
		if (at && hipMemcpyAsync(b->d_blob, b->h_blob, at, hipMemcpyHostToDevice, st) != hipSuccess) rc = -2;
	}
	if (!rc) rc = launch_pass(b, b->d_blob);
	if (rc) { (void)b->wait_stream(); end_pass(b); return rc < 0 ? rc : -2; }
	b->in_flight = true;
	return 0;
}

int cfhd_amd_decode_batch_submit_device(cfhd_amd_decode_batch *b, const void *d_base, size_t span_bytes, const size_t *offsets, const size_t *sizes, int count)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || !d_base || !offsets || !sizes || count < 1 || count > b->n || (b->groups && (count & 1))) return -1;
	for (int i = 0; i < count; i++) if (offsets[i] > span_bytes || sizes[i] > span_bytes - offsets[i]) return -1;      // a sample outside the span the caller vouched for
	(void)hipSetDevice(b->device);
	begin_pass(b, offsets, sizes, count);
	b->src_host = nullptr; b->src_device = (const uint8_t *)d_base; b->host_out = nullptr;
	if (b->groups) for (int j = 0; j < b->n; j++) b->table_src()[j] = 0;
	for (int i = 0; i < count; i++) b->table_src()[b->entry_of(i)] = offsets[i];
	const int rc = launch_pass(b, (const uint8_t *)d_base);
	if (rc) { (void)b->wait_stream(); end_pass(b); return rc < 0 ? rc : -2; }
	b->in_flight = true;
	return 0;
}

// wait of a thumbnail batch.  Final on the spot: a sample k_dec_ingest placed whose verdict has low byte 0 -- CFHD_ERROR_OKAY, its picture k_dec_thumbnail's (the scan
// flag and the colour-space tag play no part in a thumbnail).  Every other sample gets its status from CFHD_GetThumbnail on its bytes -- BADSAMPLE where that thumbnail
// has another geometry than the batch's --, and the host's picture, where there is one, takes its place in the batch's buffer, in the host pictures and, by one more
// launch of the deliver kernel per run of such neighbours, in the caller's device memory; its place stays zeros otherwise (k_dec_thumbnail wrote them, the pass
// delivered them).
static int wait_thumbnails(cfhd_amd_decode_batch *b, CFHD_Error *status)
{
	const int n = b->n, count = b->count;
	auto device_failure = [&](int code) { if (status) for (int i = 0; i < count; i++) status[i] = ERR_INTERNAL; end_pass(b); return code; };
	if (b->wait_stream()) return device_failure(-2);
	if (b->timed) {
		b->timed = false;
		float *ms[3] = { &b->ingest_ms, &b->parse_ms, &b->thumb_ms };
		for (int k = 0; k < 3; k++) if (hipEventElapsedTime(ms[k], b->ev[k], b->ev[k + 1]) != hipSuccess) { (void)hipGetLastError(); *ms[k] = 0; }
		b->deliver_ms = 0;
		if (b->deliver_timed && hipEventElapsedTime(&b->deliver_ms, b->ev[4], b->ev[5]) != hipSuccess) { (void)hipGetLastError(); b->deliver_ms = 0; }
		b->deliver_timed = false;
	}
	const int pitch = b->picture_pitch(), rows = b->picture_rows(); const size_t picture_bytes = b->picture_bytes();
	auto to_host = [&](int i, const uint8_t *picture) {
		for (int r = 0; r < rows; r++) memcpy(b->host_out + b->host_out_stride * (size_t)i + (size_t)r * b->host_out_pitch, picture + (size_t)r * pitch, (size_t)pitch);
	};
	if (b->host_out && b->thumbs_staged) parallel_for(count, count > 8 ? 8 : 1, [&](int i) { to_host(i, b->h_thumbs + picture_bytes * (size_t)i); });
	std::vector<uint8_t> bytes, scratch;
	std::vector<int> slow;                                 // the samples whose picture the host made, for the deliver kernel behind the loop
	int decoded = 0, failure = 0;
	for (int i = count; i < n; i++) b->slow_pictures[i].clear();
	for (int i = 0; i < count; i++) {
		b->slow_pictures[i].clear();
		int rc = ERR_OKAY;
		if (b->h_verdicts[n + i] || (b->h_verdicts[i] & 0xffu)) {
			const size_t size = b->full_sizes[i];
			const uint8_t *s = b->src_host ? b->src_host + b->offsets[i] : nullptr;
			if (!s) {
				bytes.resize(size ? size : 1);
				if (size && hipMemcpy(bytes.data(), b->src_device + b->offsets[i], size, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); failure = -2; }
				s = bytes.data();
			}
			// (the buffer CFHD_GetThumbnail is handed holds the thumbnail of the sample's own geometry, where its lowpass bands can lie inside the sample at all: the
			// function checks them against the size before it looks at the buffer)
			size_t need = picture_bytes, rw = 0, rh = 0, rsize = 0;
			ParsedSample own;
			if (parse_sample(s, size, &own) == 0) { const size_t w8 = (size_t)(own.width + 7) / 8, h8 = (size_t)(own.height + 7) / 8; if (w8 * h8 * 6 <= size && w8 * h8 * 4 > need) need = w8 * h8 * 4; }
			scratch.assign(need, 0);
			rc = failure ? ERR_INTERNAL : CFHD_GetThumbnail(b->slow, (void *)s, size, scratch.data(), need, 0, &rw, &rh, &rsize);
			if (rc == ERR_OKAY && (rw != (size_t)b->thumb_w || rh != (size_t)b->thumb_h)) rc = ERR_BADSAMPLE;
			b->slow_pictures[i].assign(picture_bytes, 0);
			if (rc == ERR_OKAY) memcpy(b->slow_pictures[i].data(), scratch.data(), picture_bytes);
			if (b->host_out) to_host(i, b->slow_pictures[i].data());
			(void)hipSetDevice(b->device);
			// (a synchronous copy on the null stream; the batch's stream is idle here, and the launch below is queued behind the copy's return)
			if (rc == ERR_OKAY) {
				if (hipMemcpy(b->d_thumbs + picture_bytes * (size_t)i, b->slow_pictures[i].data(), picture_bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); failure = -2; }
				if (b->dev_out) slow.push_back(i);
			}
		}
		if (status) status[i] = rc;
		decoded += rc == ERR_OKAY;
	}
	for (size_t k = 0; k < slow.size() && !failure;) {
		size_t e = k + 1;
		while (e < slow.size() && slow[e] == slow[e - 1] + 1) e++;
		if (launch_deliver(b, slow[k], (int)(e - k))) failure = -2;
		k = e;
	}
	if (!slow.empty() && !failure && b->wait_stream()) failure = -2;
	b->steps++;
	end_pass(b);
	return failure ? failure : decoded;
}

int cfhd_amd_decode_batch_wait(cfhd_amd_decode_batch *b, CFHD_Error *status)
{
	CallerDevice caller_device;
	if (!b || !b->in_flight) return -1;
	(void)hipSetDevice(b->device);
	if (b->thumbs) return wait_thumbnails(b, status);
	const int n = b->n, count = b->count;
	auto device_failure = [&](int code) { if (status) for (int i = 0; i < count; i++) status[i] = ERR_INTERNAL; end_pass(b); return code; };
	if (b->wait_stream()) return device_failure(-2);
	if (b->timed) {
		b->timed = false;
		if (hipEventElapsedTime(&b->ingest_ms, b->ev[0], b->ev[1]) != hipSuccess) { (void)hipGetLastError(); b->ingest_ms = 0; }
		if (hipEventElapsedTime(&b->blank_ms, b->ev[2], b->ev[3]) != hipSuccess) { (void)hipGetLastError(); b->blank_ms = 0; }
		b->deliver_ms = 0;      // (a pass that delivers nothing on the device has no such time)
		if (b->deliver_timed && hipEventElapsedTime(&b->deliver_ms, b->ev[4], b->ev[5]) != hipSuccess) { (void)hipGetLastError(); b->deliver_ms = 0; }
		b->deliver_timed = false;
	}
	if (b->host_out) {                                     // (pictures staged through pinned memory -- a plain buffer -- leave it on a few threads side by side; nothing to do for a registered one)
		std::atomic<int> bad(0);
		parallel_for(count, count > 8 ? 8 : 1, [&](int i) { if (b->finish_frame(i, b->host_out + b->host_out_stride * (size_t)i, b->host_out_pitch)) bad.store(1); });
		if (bad.load()) return device_failure(-2);
	}
	// the verdicts.  Final on the spot: a sample the parser refused (malformed, geometry, encoded format or channel count, bands missing) while its scan flag is the
	// prepared one -- CFHD_ERROR_BADSAMPLE, its picture already zeroed by k_dec_blank.  The slow path: what k_dec_ingest marked, what only the host parser judges, a
	// scan flag or colour-space tag other than the first sample's, and -- the band decoders' error word is one for the pass -- every sample the parser passed.
	const bool stream_damage = (b->groups ? b->gdec.batch_entropy().check() : b->dec.entropy().check()) != 0;
	const uint32_t clean = b->clean_word();
	const int picture_pitch = b->picture_pitch(); const size_t picture_bytes = b->picture_bytes();
	std::vector<uint8_t> bytes;
	int decoded = 0, failure = 0;
	std::vector<int> slow;                                 // the samples the handle decoded, for k_dec_deliver behind the loop
	std::vector<int> slow_mode;                            // ... and, for the RGB_AS_* layouts, what each is delivered as: its own sample's matrix, or zeros where the handle refused it
	const bool rgb_as_yuv = b->dev_out && dev::deliver_is_rgb_as_yuv(b->dev_out_layout);
	for (int i = count; i < n; i++) b->slow_pictures[i].clear();      // (a short pass: what an earlier pass left behind its count is that pass's picture in HBM again)
	for (int i = 0; i < count; i++) {
		uint32_t v = b->h_verdicts[i], mark = b->h_verdicts[n + i];
		if (b->groups) {
			// a pair is judged alone and as one, entry 2 g and entry 2 g + 1 alike: final where both samples were placed, the follower is a clean P-frame sample and
			// the group is clean -- both OKAY -- or failed the parser for a reason the handle calls a bad sample -- both BADSAMPLE: a follower without its group has
			// no picture on the handle either --; the slow handle, which forgets its last group in front of the pair, otherwise
			const int g = i >> 1, ng = b->ngroups;
			v = b->h_verdicts[g]; mark = b->h_verdicts[n + g] | b->h_verdicts[n + ng + g] | b->h_verdicts[ng + g];
			if (!(i & 1)) decoder_group_reset(b->slow);
		}
		const int reason = (int)(v & 0xffu);
		const bool scan_as_prepared = ((v >> 8) & 1u) == (b->st.progressive_flag ? 1u : 0u);
		b->slow_pictures[i].clear();
		int rc;
		if (!mark && reason >= dev::DEC_VERDICT_MALFORMED && reason <= dev::DEC_VERDICT_BANDS && scan_as_prepared) rc = ERR_BADSAMPLE;
		else if (!mark && v == clean && !stream_damage) rc = ERR_OKAY;
		else {
			const size_t size = b->full_sizes[i];
			const uint8_t *s = b->src_host ? b->src_host + b->offsets[i] : nullptr;
			if (!s) {
				bytes.resize(size ? size : 1);
				if (size && hipMemcpy(bytes.data(), b->src_device + b->offsets[i], size, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); failure = -2; }
				s = bytes.data();
			}
			// the handle's picture is kept with the batch whichever way the pass delivers its pictures: download_output(i) then agrees with status[i], not with what the
			// device stage left in HBM
			b->slow_pictures[i].assign(picture_bytes, 0);
			rc = failure ? ERR_INTERNAL : CFHD_DecodeSample(b->slow, (void *)s, size, b->slow_pictures[i].data(), picture_pitch);
			if (b->host_out) for (int r = 0; r < b->picture_rows(); r++)
				memcpy(b->host_out + b->host_out_stride * (size_t)i + (size_t)r * b->host_out_pitch, b->slow_pictures[i].data() + (size_t)r * picture_pitch, (size_t)picture_pitch);
			(void)hipSetDevice(b->device);
			// ... and what the caller's device memory holds agrees with it too: the handle's picture (zeros where it refused) takes the sample's place in the batch's own
			// buffer, k_dec_deliver runs again below.  (A synchronous copy out of pageable memory on the null stream: the launch below, on the batch's stream, is ordered
			// behind it only because hipMemcpy returns when the bytes are in HBM -- the batch's stream is idle here, wait_stream() above.)
			if (b->dev_out) {
				if (hipMemcpy(b->device_pictures() + picture_bytes * (size_t)i, b->slow_pictures[i].data(), picture_bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); failure = -2; }
				slow.push_back(i);
				int mode = dev::RGB_AS_YUV_ZERO;
				if (rgb_as_yuv && rc == ERR_OKAY) { ParsedSample own; mode = dev::deliver_rgb_as_yuv_mode(parse_sample(s, size, &own) >= 0 ? own.color_space : 0); }
				slow_mode.push_back(rgb_as_yuv ? mode : -1);
			}
		}
		if (status) status[i] = rc;
		decoded += rc == ERR_OKAY;
	}
	// one launch per run of neighbouring slow samples (a damaged code stream: one run, the whole pass; the RGB_AS_* layouts: neighbours of one mode), then one wait
	for (size_t k = 0; k < slow.size() && !failure;) {
		size_t e = k + 1;
		while (e < slow.size() && slow[e] == slow[e - 1] + 1 && slow_mode[e] == slow_mode[k]) e++;
		if (launch_deliver(b, slow[k], (int)(e - k), slow_mode[k])) failure = -2;
		k = e;
	}
	if (!slow.empty() && !failure && b->wait_stream()) failure = -2;
	b->steps++;
	end_pass(b);
	return failure ? failure : decoded;
}

int cfhd_amd_decode_batch_download_output(cfhd_amd_decode_batch *b, int i, void *out, int pitch)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || i < 0 || i >= b->n || !out || pitch < b->picture_pitch()) return -1;
	const int rows = b->picture_rows(), row_bytes = b->picture_pitch();
	if (!b->slow_pictures[i].empty()) {                    // decoded by the slow path of the last pass
		for (int r = 0; r < rows; r++) memcpy((uint8_t *)out + (size_t)r * pitch, b->slow_pictures[i].data() + (size_t)r * row_bytes, (size_t)row_bytes);
		return 0;
	}
	if (b->thumbs) {                                       // the DPX0 words out of the batch's own buffer
		(void)hipSetDevice(b->device);
		if (hipMemcpy2DAsync(out, (size_t)pitch, b->d_thumbs + b->picture_bytes() * (size_t)i, (size_t)row_bytes, (size_t)row_bytes, (size_t)rows, hipMemcpyDeviceToHost, (hipStream_t)b->stream()) != hipSuccess) { (void)hipGetLastError(); return -2; }
		return b->wait_stream();
	}
	if (b->download_frame(i, out, pitch) || b->wait_stream()) return -2;
	return b->finish_frame(i, out, pitch);
}

// which: 0 k_dec_ingest, 1 k_dec_parse, 2 the band decoder (all its kernels), 3 k_dec_lowpass, 4 / 5 / 6 the transform levels in launch order (wavelet 3, wavelet 2, the
// last level + output conversion), 7 k_dec_blank, 9 k_dec_deliver -- both kinds of batch; 0 when the last pass delivered nothing on the device -- (ms of the last pass,
// HIP events on the batch's stream)
float cfhd_amd_decode_batch_kernel_ms(cfhd_amd_decode_batch *b, int which)
{
	if (b && !b->in_flight && which == 9) return b->deliver_ms;
	// a batch of thumbnails: 0 k_dec_ingest, 1 k_dec_parse, 6 k_dec_thumbnail (the place of the last level), nothing else
	if (b && !b->in_flight && b->thumbs) return which == 0 ? b->ingest_ms : (which == 1 ? b->parse_ms : (which == 6 ? b->thumb_ms : 0));
	if (!b || b->in_flight || which < 0 || which > (b->groups ? 8 : 7)) return 0;
	if (which == 0) return b->ingest_ms;
	if (which == 7) return b->blank_ms;
	// a batch of groups: 1 k_dec_parse_group, 2 the band decoder (every kernel of it), 3 k_dec_lowpass, 4 / 5 / 6 GopBatch's inverse stages in launch order (the top wavelet;
	// the two middle wavelets + the temporal step; the last level of all frames + the output conversion), and 8: k_dec_band_two_pass alone
	if (b->groups) return which == 8 ? b->gdec.batch_entropy().kernel_ms(3) : (which < 4 ? b->gdec.batch_entropy().kernel_ms(which - 1) : b->gdec.stage_ms(6 - which));
	if (which < 4) return b->dec.entropy().kernel_ms(which - 1);
	return b->dec.last_level_ms(6 - which);
}

const char *cfhd_amd_decode_batch_kernel_name(cfhd_amd_decode_batch *b, int which)
{
	if (b && !b->in_flight && b->thumbs) return which == 0 ? "k_dec_ingest" : (which == 1 ? "k_dec_parse" : (which == 6 ? "k_dec_thumbnail" : (which == 9 && b->dev_out ? (dev::deliver_is_rgb10(b->dev_out_layout) ? "k_dec_deliver_rgb10" : "k_dec_deliver") : "")));
	if (b && !b->in_flight && which == 9) return b->dev_out && dev::deliver_is_bayer(b->dev_out_layout) ? "k_dec_deliver_bayer" : (b->dev_out && dev::deliver_is_yuv422(b->dev_out_layout) ? "k_dec_deliver_yuv422" : (b->dev_out && dev::deliver_is_rgba(b->dev_out_layout) ? "k_dec_deliver_rgba" : (b->dev_out && dev::deliver_is_rgb_as_yuv(b->dev_out_layout) ? "k_dec_deliver_rgb_as_yuv" : "k_dec_deliver")));
	if (!b || b->in_flight || which < 0 || which > 7) return "";
	static const char *const fixed[4] = { "k_dec_ingest", "k_dec_parse", "k_dec_plan+k_dec_index+k_dec_chain+k_dec_tiles", "k_dec_lowpass" };
	if (which < 4 && !(b->groups && which)) return fixed[which];
	if (which == 7) return "k_dec_blank";
	if (b->groups) return which == 1 ? "k_dec_parse_group" : (which == 2 ? b->band_name : (which == 3 ? fixed[3] : b->gdec.stage_kernel(6 - which)));
	return b->dec.level_kernel(6 - which);
}

} // extern "C"
