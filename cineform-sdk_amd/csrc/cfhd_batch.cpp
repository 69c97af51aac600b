// cfhd_batch.cpp -- device-resident batched round trip (extension API, cfhd_amd_batch_*), used by bench.py and by
// callers that keep frames in HBM: N frames -> forward kernels -> entropy coding -> N samples -> entropy decoding
// -> inverse kernels -> N frames in HBM.  One launch per stage covers the whole batch.
//
// Default: every stage on the GPU; the decoder reads the samples where the encoder left them in HBM (k_dec_parse) while their
// host copy travels beside it.  CFHD_AMD_HANDOFF=host sends the samples through the host parser and back;
// CFHD_AMD_ENTROPY=host keeps the run-length/VLC stage on host threads (the reference's own arrangement, Codec/encoder.c:5386 /
// decoder.c:19534), fed by one D2H copy of the quantized bands and followed by one H2D copy of the dequantized bands.
//
// Two-frame groups (CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP): a batch of nframes / 2 groups, frames 2 g and 2 g + 1 forming group g, through two GopBatch objects (encoder |
// decoder) in the default arrangement only -- every stage on the GPU, the group samples parsed where the coder left them (k_dec_parse_group), one chunk, no host wait
// between submit and wait.  The P-frame samples and the sequence header are host code.  cfhd_amd_batch_create_group_stream: the same batch as one group encoder's
// stream, tables that follow the key samples included (Stream, GroupUnits).
#include "../../include/cfhd_amd.h"
#include "cfhd_core.h"
#include "cfhd_bitstream.h"
#include "cfhd_device.h"
#include "cfhd_metadata.h"
#include "cfhd_params.h"
#include "cfhd_gop.h"
#include <string.h>
#include <stdlib.h>
#include <vector>
#include <thread>
#include <atomic>
#include <chrono>
#include <memory>

using namespace cfhd;

struct cfhd_amd_chunk { EncodeBatch enc; DecodeBatch dec; int first = 0, n = 0; };
enum { kPFrameSampleBytes = 24, kSequenceHeaderBytes = 40 };

struct cfhd_amd_batch {
	FramePlan plan;
	int n = 0, nthreads = 1, quality = 4, pixel_kind = PIX_YUY2;
	int color_format = 2, color_space = 2; bool progressive = true;
	bool decode = true;                // false: encode only (cfhd_amd_batch_create_ex mode 1: the Avid 4:2:2 layouts and BYR5, which no decoder output has; BYR4 round trips through cfhd_amd_batch_create_bayer)
	// The batch is cut into chunks with their own HIP streams: while one chunk's entropy decode (latency bound: one lane per
	// band) is in flight, the next chunk's bandwidth-bound kernels and PCIe copies run beside it.
	std::vector<std::unique_ptr<cfhd_amd_chunk>> chunks;
	cfhd_amd_chunk &chunk_of(int i, int *local) { for (auto &c : chunks) if (i < c->first + c->n) { *local = i - c->first; return *c; } *local = 0; return *chunks[0]; }
	std::vector<std::vector<uint8_t>> samples;
	std::vector<size_t> sample_size;
	MetaState meta;                    // the metadata a synchronous encoder attaches on its own (SampleEncoder.cpp:744-939): frame i of the batch = the (steps * n + i + 1)-th CFHD_EncodeSample call
	std::vector<MetaBlock> frame_meta;  // per frame: the global block as it stood when the frame was "submitted"
	uint32_t steps = 0;
	bool gpu_entropy = true;
	bool device_handoff = true;        // the decoder reads the samples where the encoder left them in HBM (k_dec_parse); the host copy arrives beside it
	double t_fwd = 0, t_entropy_enc = 0, t_entropy_dec = 0, t_inv = 0;   // wall seconds of the last round trip
	// the frame queue (cfhd_amd_batch_submit / _wait): the pass in flight runs on a thread of its own, on the batch's own HIP streams
	// (cfhd_amd_batch_submit / _wait).  The default arrangement -- everything on the GPU, one chunk -- needs no thread: submit queues the whole pass on the batch's streams
	// (the decoder's stream waits for the encoder's events), wait fetches the sizes, queues the copy of the samples and waits for both streams.  The other arrangements
	// (host hand-off, host entropy, several chunks) have host work in the middle of a pass: those run the blocking pass on a thread of their own.
	std::thread worker; bool in_flight = false, queued = false; long long pending = -1;
	bool counted = false;              // the pass in flight is one of its device's passes in flight (cfhd_device.h device_pass_begin; pass_counted below)
	// cfhd_amd_batch_submit_host: the pass in flight takes its frames from / leaves its pictures in the caller's memory
	const uint8_t *host_in = nullptr; size_t host_in_stride = 0; int host_in_pitch = 0;
	uint8_t *host_out = nullptr; size_t host_out_stride = 0; int host_out_pitch = 0;
	double t_launch0 = 0, t_launched = 0;
	std::vector<void *> shared_streams;      // streams several objects of the batch share (StreamScope): released behind the objects
	// two-frame groups: n / 2 groups on one encoder and (round trips) one decoder object; `chunks` stays empty.  Sample 2 g is group g, sample 2 g + 1 the 24-byte
	// P-frame sample behind it; both carry frame number steps * n + 2 g + 1, as one CFHD_EncodeSample handle numbers them
	bool gop = false; GopPlan gplan;
	std::unique_ptr<GopBatch> genc, gdec;
	std::vector<uint8_t> pframes; uint8_t sequence_header[64]; size_t sequence_header_size = 0;
	int ngroups() const { return n / 2; }
	// cfhd_amd_batch_create_stream: the batch is one encoder's stream, pass behind pass -- frame i of pass k is call k n + i + 1 of one CFHD_EncodeSample handle, rate
	// feedback included.  moving: the quality's tables follow the size of the sample in front (encode_one, cfhd_api_params.h); then every frame carries tables of its
	// own, a pass is coded on a guess of them and the frames from the first wrong guess on are coded again (stream_rounds).  The state below is the handle's
	// EncodeParams::qstate / plan, held at the pass boundary; a pass that fails leaves it alone.
	// cfhd_amd_batch_create_group_stream: the same for two-frame groups -- "frame" reads "group" (a unit of the pass), the handle is one that was prepared with the group
	// flag, its state EncodeParams::gstate / gplan, the size that feeds back the one of the key sample in front (the group sample; the sequence header for the first).
	template <typename Plan> struct StreamTables {
		Plan carried_plan;                              // the tables of the last unit of the last completed pass (before the first pass: the tables CFHD_PrepareToEncode derives)
		std::vector<Plan> coded;                        // the tables unit i was coded with last: a pass's guess, then its result, then the next pass's guess
	};
	struct Stream {
		bool on = false, moving = false;
		int derive_quality = 0;                         // the quality word derive_quantization takes (the caller's with the format marks)
		QuantState carried = {0, -1, 0};                // behind the last unit of the last completed pass
		size_t carried_bytes = 0;                       // that unit's sample size (0: none yet -- the first frame of a stream derives nothing)
		StreamTables<FramePlan> frames; StreamTables<GopPlan> groups;      // (the one the batch's units are)
		std::vector<QuantState> before;                 // the state in front of unit i's derivation, as far as the pass is verified
		QuantState next = {0, -1, 0};                   // what a pass that ends well carries on
		int rounds = 0, frames_coded = 0, stats[3] = {0, 0, 0}; bool stats_valid = false;
	} stream;
	~cfhd_amd_batch() { if (worker.joinable()) worker.join(); chunks.clear(); genc.reset(); gdec.reset(); for (void *s : shared_streams) device_stream_release(s); }
};

namespace {
cfhd_amd_batch *create_intra_batch(const FrontEndParams &fp, int width, int height, int nframes, int nthreads, int mode, bool stream, bool bayer_round_trip = false);
template <typename F> void parallel_for(int n, int nthreads, F f)
{
	if (nthreads <= 1 || n <= 1) { for (int i = 0; i < n; i++) f(i); return; }
	std::atomic<int> next(0);
	std::vector<std::thread> pool;
	int t = nthreads < n ? nthreads : n;
	for (int k = 0; k < t; k++) pool.emplace_back([&] { for (int i; (i = next.fetch_add(1)) < n;) f(i); });
	for (auto &th : pool) th.join();
}
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The frame queue's pass joins (submit, in front of its first launch) / leaves (wait, or a submit that fails) the passes in flight on its device: launches of this and
// of other queues size their persistent kernels by that count (GpuEntropyDecoder::launch_dx).  The batch's own decoders are told that their pass is in it.
// (The device is the encoder's: a batch prepares its encoder and its decoder on one device, the one launch_dx reads the count of.  Group batches count too,
// though their own band decoder has no persistent kernels: they are passes that want room beside an intra batch's.)
void pass_counted(cfhd_amd_batch *b, bool on)
{
	if (b->counted == on) return;
	const int device = b->gop ? b->genc->device() : b->chunks[0]->enc.device();
	if (on) device_pass_begin(device); else device_pass_end(device);
	for (auto &c : b->chunks) c->dec.entropy().set_pass_counted(on);
	b->counted = on;
}
// a submit: counted from here on; every return that does not keep() the pass -- a launch that failed -- takes it out of the count again
struct CountedSubmit {
	cfhd_amd_batch *b; bool kept = false;
	explicit CountedSubmit(cfhd_amd_batch *batch) : b(batch) { pass_counted(b, true); }
	~CountedSubmit() { if (!kept) pass_counted(b, false); }
	int keep(bool queued) { kept = true; b->in_flight = true; b->queued = queued; return 0; }
	CountedSubmit(const CountedSubmit &) = delete;
};

// ---- streams with rate feedback (cfhd_amd_batch_create_stream, tables that move)
bool same_tables(const FramePlan &a, const FramePlan &b)      // (tables, not states: two states can give the same divisors)
{
	for (int c = 0; c < a.num_channels; c++)
		for (int lv = 0; lv < kNumLevels; lv++)
			for (int k = 0; k < kNumBands; k++) if (a.ch[c].band[lv][k].quant != b.ch[c].band[lv][k].quant) return false;
	return true;
}
// One step of the handle's walk (encode_one): `plan` holds the tables of the frame in front and becomes this frame's, derived from the size of that frame's sample --
// or stays, when there is no such sample (the first frame of a stream).
void stream_step(const cfhd_amd_batch *b, QuantState *st, size_t bytes_in_front, FramePlan *plan)
{
	st->lastgopbitcount = (int64_t)bytes_in_front * 8;
	if (st->lastgopbitcount) derive_quantization(plan, b->stream.derive_quality, b->progressive, 0.0f, st);
}
SampleHeaderInfo stream_header(const cfhd_amd_batch *b, int i)
{
	SampleHeaderInfo h = { b->steps * (uint32_t)b->n + (uint32_t)i + 1, b->color_format, b->color_space, b->quality, b->progressive, b->frame_meta[i].data(), b->frame_meta[i].size(), nullptr, 0 };
	return h;
}
// The header of group g's sample: the number and the metadata of the handle's call that completes the group (gop_launch deals the blocks, one per frame and pass)
SampleHeaderInfo group_header(const cfhd_amd_batch *b, int g)
{
	const MetaBlock &m = b->frame_meta[2 * g + 1];
	SampleHeaderInfo h = { b->steps * (uint32_t)b->n + 2u * (uint32_t)g + 1u, b->color_format, b->color_space, b->quality, b->progressive, m.data(), m.size(), nullptr, 0 };
	return h;
}
uint32_t pass_seed(const cfhd_amd_batch *b) { return 0xA511E9B3u * (b->steps + 1); }

// What the passes of a stream ask of their units: the frames of an intra batch (FrameUnits) or the groups of a group batch (GroupUnits).  stream_begin_pass,
// stream_rounds and stream_end_pass below are written once against these.
struct FrameUnits {
	typedef FramePlan Plan;
	cfhd_amd_batch *b; cfhd_amd_chunk *c;
	explicit FrameUnits(cfhd_amd_batch *batch) : b(batch), c(batch->chunks[0].get()) {}
	int count() const { return b->n; }
	int frames_per_unit() const { return 1; }
	cfhd_amd_batch::StreamTables<Plan> &tables() const { return b->stream.frames; }
	GpuEntropyEncoder &entropy() const { return c->enc.entropy(); }
	static bool same(const Plan &x, const Plan &y) { return same_tables(x, y); }
	bool step(QuantState *st, size_t bytes_in_front, Plan *plan, int) const { stream_step(b, st, bytes_in_front, plan); return true; }
	const Plan &device_plan(int i) const { return c->enc.frame_plan(i); }
	int set_tables(int i, const Plan &p) const { return c->enc.set_frame_quant(i, p); }
	int set_header(int i, const Plan &p) const { entropy().set_plan(p); return entropy().set_frame_header(i, stream_header(b, i)); }      // (the header carries the unit's own tables)
	bool spoils_the_pass(int i) const { return !entropy().sample_bytes(i); }      // (a final sample that does not fit its buffer: -3)
	int launch_window(int first, int n) const { return c->enc.launch_forward(false, first, n); }
	int encoder_wait() const { return c->enc.wait(); }
	int decoder_wait() const { return c->dec.wait(); }
	int decode_again() const                            // the decoder's half over the final samples
	{
		GpuEntropyEncoder &ent = entropy();
		c->dec.entropy().set_producer_events(ent.headers_event(), ent.samples_event());
		if (c->dec.entropy().set_samples_device(ent.device_samples(), 0, ent.device_sizes(), ent.device_offsets())) return -4;
		if (c->dec.launch_entropy() || c->dec.launch_inverse(pass_seed(b) + (uint32_t)c->first)) return -5;
		if (b->host_out && c->dec.download_frames(b->host_out, b->host_out_stride, b->host_out_pitch)) return -5;
		return 0;
	}
	size_t last_sample_bytes() const { return b->sample_size[b->n - 1]; }
};
struct GroupUnits {
	typedef GopPlan Plan;
	cfhd_amd_batch *b;
	explicit GroupUnits(cfhd_amd_batch *batch) : b(batch) {}
	int count() const { return b->ngroups(); }
	int frames_per_unit() const { return 2; }
	cfhd_amd_batch::StreamTables<Plan> &tables() const { return b->stream.groups; }
	GpuEntropyEncoder &entropy() const { return b->genc->entropy(); }
	static bool same(const Plan &x, const Plan &y) { return gop_same_tables(x, y); }
	// the two calls of the handle that make group g (cfhd_gop.h gop_quant_group), on the bytes of the key sample in front; the stream's first group: on none, the
	// sequence header lying between its two calls
	bool step(QuantState *st, size_t bytes_in_front, Plan *plan, int g) const
	{
		gop_quant_key_sample(st, bytes_in_front);
		return gop_quant_group(plan, b->stream.derive_quality, st, b->steps == 0 && g == 0, kSequenceHeaderBytes);
	}
	const Plan &device_plan(int g) const { return b->genc->group_plan(g); }
	int set_tables(int g, const Plan &p) const { return b->genc->set_group_plan(g, p); }
	int set_header(int g, const Plan &p) const { entropy().set_group_plan(p); return entropy().set_frame_header(g, group_header(b, g)); }
	// (-3, and -9: the handle would hand such a group to the host writer, whose sample the device stage cannot give -- gop_finish fails the pass)
	bool spoils_the_pass(int g) const { const size_t n = entropy().sample_bytes(g); return !n || gop_sample_may_zero_bands(b->gplan, n); }
	int launch_window(int first, int n) const { return b->genc->launch_forward(first, n); }
	int encoder_wait() const { return b->genc->wait(); }
	int decoder_wait() const { return b->gdec->wait(); }
	int decode_again() const
	{
		GpuEntropyEncoder &ent = entropy(); GopBatch &dec = *b->gdec;
		dec.batch_entropy().set_producer_events(ent.headers_event(), ent.samples_event());
		if (dec.batch_entropy().set_samples_device(ent.device_samples(), ent.device_sizes(), ent.device_offsets())) return -4;
		if (dec.batch_entropy().launch() || dec.launch_inverse(pass_seed(b), true)) return -5;
		if (b->host_out && dec.download_frames(b->host_out, b->host_out_stride, b->host_out_pitch)) return -5;
		return 0;
	}
	size_t last_sample_bytes() const { return b->sample_size[b->n - 2]; }
};

// Round 0 of a pass: unit 0 carries the tables the carried state gives it, the units behind it a guess -- in the first pass the same tables, afterwards the tables
// the last pass ended with, unit by unit (on ordinary material the tables stand still for long runs, and a cut that repeats -- a loop, a benchmark -- repeats them).
template <typename Units> int stream_begin_pass(const Units &u)
{
	cfhd_amd_batch *b = u.b;
	cfhd_amd_batch::Stream &s = b->stream;
	std::vector<typename Units::Plan> &coded = u.tables().coded;
	s.rounds = 1; s.frames_coded = b->n;
	QuantState st = s.carried; typename Units::Plan first = u.tables().carried_plan;
	if (!u.step(&st, s.carried_bytes, &first, 0)) return -2;
	for (int i = 0; i < u.count(); i++) {
		const typename Units::Plan &guess = i && b->steps ? coded[i] : first;
		if (Units::same(guess, u.device_plan(i))) { coded[i] = u.device_plan(i); continue; }
		coded[i] = guess;
		if (u.set_tables(i, guess)) return -2;
	}
	return 0;
}
// The rounds behind round 0, with the sizes of the round before on the host and the encoder's stream drained.  The walk starts at the first frame whose tables are not
// verified yet, j, with the state in front of it, and derives every frame's tables from the size of the sample in front -- the handle's own steps.  Up to the first frame
// whose tables differ from the ones it was coded with, every sample is the handle's: sample i - 1 final makes the tables of frame i final.  That frame and the ones behind
// it get the tables the walk has found (a guess again behind the first) and are coded again, as a window of the batch; j rises every round, so a pass takes at most n
// rounds and ends on the handle's samples.  The metadata blocks are the ones batch_launch dealt: one per frame and pass.  Returns 0 -- also for a pass that batch_finish
// is about to fail (a verified frame that does not fit) -- or < 0.
template <typename Units> int stream_rounds(const Units &u)
{
	typedef typename Units::Plan Plan;
	cfhd_amd_batch *b = u.b;
	cfhd_amd_batch::Stream &s = b->stream;
	std::vector<Plan> &coded = u.tables().coded;
	GpuEntropyEncoder &ent = u.entropy();
	const int n = u.count();
	std::vector<Plan> found((size_t)n);
	bool recoded = false;
	s.before[0] = s.carried;
	for (int j = 0;;) {
		QuantState st = s.before[j]; Plan plan = j ? coded[j - 1] : u.tables().carried_plan;
		int wrong = -1;
		for (int i = j; i < n; i++) {
			const size_t in_front = i ? ent.sample_bytes(i - 1) : s.carried_bytes;
			if (wrong < 0 && i && u.spoils_the_pass(i - 1)) return 0;      // (sample i - 1 is final, and fails the pass)
			if (wrong < 0) s.before[i] = st;
			if (!u.step(&st, in_front, &plan, i)) return -2;
			if (wrong < 0 && !Units::same(plan, coded[i])) wrong = i;
			found[i] = plan;
		}
		if (wrong < 0) { s.next = st; break; }
		// (mode 0: the decoder of the round before is reading the dense buffer the coder is about to write again)
		if (b->decode && u.decoder_wait()) return -5;
		for (int i = wrong; i < n; i++) {
			coded[i] = found[i];
			if (u.set_tables(i, found[i])) return -2;
			if (u.set_header(i, found[i])) return -6;
		}
		const int count = n - wrong;
		if (u.launch_window(wrong, count) || ent.launch(wrong, count) || ent.download_queue(wrong, count) || ent.download_finish(wrong, count) || u.encoder_wait()) return -2;
		s.rounds++; s.frames_coded += count * u.frames_per_unit(); recoded = true;
		j = wrong;
	}
	if (recoded && b->decode) return u.decode_again();
	return 0;
}
// A pass that ended well: its last unit is what the next pass goes on from.  stats: rounds, frames coded over all rounds, units whose tables differ from those of
// the unit in front (unit 0: from the last unit of the pass before; in a stream's first pass it has none in front).
template <typename Units> void stream_end_pass(const Units &u)
{
	cfhd_amd_batch *b = u.b;
	cfhd_amd_batch::Stream &s = b->stream;
	if (!s.moving) { s.stats[0] = 1; s.stats[1] = b->n; s.stats[2] = 0; s.stats_valid = true; return; }
	const std::vector<typename Units::Plan> &coded = u.tables().coded;
	int moved = 0;
	for (int i = 0; i < u.count(); i++) moved += (i || b->steps) && !Units::same(coded[i], i ? coded[i - 1] : u.tables().carried_plan);
	s.stats[0] = s.rounds; s.stats[1] = s.frames_coded; s.stats[2] = moved; s.stats_valid = true;
	s.carried = s.next; u.tables().carried_plan = coded[u.count() - 1]; s.carried_bytes = u.last_sample_bytes();
}

// The default pass (all stages on the GPU, samples handed over in HBM, one chunk) in two halves with no host wait inside either.
// batch_launch: every launch of the pass queued -- forward transform, entropy coder, dense copy of the samples + their sizes on the way to the host on the encoder's
// stream; parser, entropy decoder and inverse transform on the decoder's stream behind the encoder's events (headers final / payloads final).  Returns 0 or < 0.
int batch_launch(cfhd_amd_batch *b)
{
	cfhd_amd_chunk *c = b->chunks[0].get();
	b->t_launch0 = now();
	c->enc.collect_begin_pass();                        // (the k_enc_collect launches that fed this pass, if any: cfhd_amd_batch_kernel_ms index 20)
	const uint32_t base_number = b->steps * (uint32_t)b->n;
	// every frame gets the metadata CFHD_EncodeSample would give it: GUID, encode date / time, a timecode and a unique frame number that advance per frame
	b->frame_meta.resize(b->n);
	for (int i = 0; i < b->n; i++) { b->meta.handle(); b->frame_meta[i] = b->meta.global; meta_remove_hidden(b->frame_meta[i]); }
	const uint32_t seed = 0xA511E9B3u * (b->steps + 1);
	if (b->stream.moving && stream_begin_pass(FrameUnits(b))) return -2;
	// Encode-only passes in flight on one device take turns (cfhd_device.h stage_order_wait): this pass's forward transform starts behind the entropy coder of the pass
	// queued before it.  Passes that start together otherwise run in lock step -- all encode, then all copy their samples to the host, and the copies (the PCIe link) and
	// the kernels never overlap: byr4-2160p 18.9 k fps with turns, 11.9 k without; rg48-2160p 15.9 / 12.4 k.  Round-trip passes run free: their decode halves fill the
	// gaps, and turns -- for the encode halves alone or for both -- cost 6 % (54.6 vs 58.1 k fps at 1080p, 16.5 vs 17.9 k at 2160p, 51.4 vs 55.8 k at 1080i; 16 hardware
	// queues, three steps in flight: profiles/r05_o_*).  CFHD_AMD_QUEUE=ordered: (A/B) turns for both halves of every pass; =free: for none.
	static const int forced = [] { const char *e = getenv("CFHD_AMD_QUEUE"); return e && strcmp(e, "ordered") == 0 ? 2 : (e && strcmp(e, "free") == 0 ? 0 : -1); }();
	const int turns = forced >= 0 ? forced : (b->decode ? 0 : 1);
	const bool ordered = turns >= 1, ordered_decode = turns >= 2;
	if (ordered && stage_order_wait(c->enc.device(), 0, c->enc.stream())) return -2;
	// fed from the host: the frames' copies first, on the encoder's stream (passes in flight on other batches run beside them)
	if (b->host_in && c->enc.upload_frames(b->host_in, b->host_in_stride, b->host_in_pitch)) return -2;
	// the transform kernels start first: the host serialises the sample headers (0.5 ms per 256) while they run
	if (c->enc.launch_forward(false)) return -2;         // (nothing but the entropy stage reads these coefficients)
	for (int l = 0; l < c->n; l++) {
		SampleHeaderInfo h = { base_number + (uint32_t)(c->first + l) + 1, b->color_format, b->color_space, b->quality, b->progressive, b->frame_meta[c->first + l].data(), b->frame_meta[c->first + l].size(), nullptr, 0 };
		if (b->stream.moving) c->enc.entropy().set_plan(b->stream.frames.coded[l]);      // (the header carries the frame's own tables)
		if (c->enc.entropy().set_frame_header(l, h)) return -6;
	}
	if (c->enc.entropy().launch()) return -2;
	if (ordered && stage_order_done(c->enc.device(), 0, c->enc.stream())) return -2;      // (in front of the copies to the host: the next pass's encode does not wait for PCIe)
	if (b->decode) {
		if (ordered_decode && stage_order_wait(c->enc.device(), 1, c->dec.stream())) return -5;
		// the parser only needs the headers and size fields (k_ent_layout): it runs beside k_ent_emit, the band decoder waits for the payloads
		c->dec.entropy().set_producer_events(c->enc.entropy().headers_event(), c->enc.entropy().samples_event());
		if (c->dec.entropy().set_samples_device(c->enc.entropy().device_samples(), 0, c->enc.entropy().device_sizes(), c->enc.entropy().device_offsets())) return -4;
		if (c->dec.launch_entropy() || c->dec.launch_inverse(seed + (uint32_t)c->first)) return -5;
		if (ordered_decode && stage_order_done(c->enc.device(), 1, c->dec.stream())) return -5;
		if (b->host_out && c->dec.download_frames(b->host_out, b->host_out_stride, b->host_out_pitch)) return -5;      // the pictures' copies behind the inverse transform, on the decoder's stream
	}
	if (c->enc.entropy().download_queue()) return -2;
	b->t_launched = now();
	return 0;
}
// batch_finish: the sizes arrive, the copy of the sample bytes is queued, both streams drain.  Returns the total number of sample bytes or < 0.
long long batch_finish(cfhd_amd_batch *b)
{
	cfhd_amd_chunk *c = b->chunks[0].get();
	if (c->enc.entropy().download_finish() || c->enc.wait()) return -2;
	// a stream whose tables move: the sizes say whether the guess of the tables held; if not, the frames behind the first wrong one are coded again (no turns taken:
	// stage_order_wait is round 0's)
	if (b->stream.moving) { const int rc = stream_rounds(FrameUnits(b)); if (rc) return rc; }
	// A frame whose sample does not fit its buffer has size 0 (k_ent_layout) and fails the pass with -3 -- behind the loop: the samples of the other frames are complete
	// and keep their sizes for cfhd_amd_batch_get_sample, and the decoder's stream, which is parsing these buffers, has drained before the caller gets the batch back.
	bool overflow = false, peaks = false;
	for (int l = 0; l < c->n; l++) {
		size_t n = c->enc.entropy().sample_bytes(l); b->sample_size[c->first + l] = n;
		if (!n) { overflow = true; continue; }
		if (c->enc.entropy().needs_peak_table(l)) peaks = true;   // a band with more peak values than the entropy stage's positions hold (two million): only CFHD_EncodeSample writes such a sample (host writer)
	}
	const double t_enc = now();
	if (b->decode && c->dec.wait()) return -5;
	if (overflow) return -3;
	if (peaks) return -8;
	if (b->decode && c->dec.entropy().check()) return -7;
	if (b->decode && b->host_out) {                  // (pictures staged through pinned memory -- a plain buffer -- leave it on a few threads side by side; nothing to do for a registered one)
		std::atomic<int> bad(0);
		parallel_for(c->n, c->n > 8 ? 8 : 1, [&](int l) { if (c->dec.finish_frame(l, b->host_out + b->host_out_stride * (size_t)l, b->host_out_pitch)) bad.store(1); });
		if (bad.load()) return -5;
	}
	const double t4 = now();
	b->t_fwd = b->t_launched - b->t_launch0; b->t_entropy_enc = t_enc - b->t_launched; b->t_entropy_dec = 0; b->t_inv = t4 - t_enc;
	if (b->stream.on) stream_end_pass(FrameUnits(b));
	b->steps++;
	long long total = 0;
	for (int i = 0; i < b->n; i++) total += (long long)b->sample_size[i];
	return total;
}

// The same two halves for a batch of two-frame groups.  gop_launch: (frames from the host,) level 1 of all frames, temporal step and the three spatial wavelets, the
// entropy coder over the n / 2 group samples -- their headers serialised on the host while the transforms run --; on the decoder's stream the parser behind the coder's
// headers, the band decoder behind its payloads, the inverse transforms, (the pictures to the host).  Nothing waits.
int gop_launch(cfhd_amd_batch *b)
{
	GopBatch &enc = *b->genc;
	const int ng = b->ngroups();
	b->t_launch0 = now();
	enc.collect_begin_pass();                           // (the k_enc_collect launches that fed this pass, if any: cfhd_amd_batch_kernel_ms index 20)
	// the metadata of the handle's call that completes group g: CFHD_EncodeSample advances it on every call, frame by frame
	b->frame_meta.resize(b->n);
	for (int i = 0; i < b->n; i++) { b->meta.handle(); b->frame_meta[i] = b->meta.global; meta_remove_hidden(b->frame_meta[i]); }
	const uint32_t seed = 0xA511E9B3u * (b->steps + 1);
	static const int forced = [] { const char *e = getenv("CFHD_AMD_QUEUE"); return e && strcmp(e, "ordered") == 0 ? 2 : (e && strcmp(e, "free") == 0 ? 0 : -1); }();
	const int turns = forced >= 0 ? forced : (b->decode ? 0 : 1);      // (encode-only passes take turns, round trips run free: batch_launch says why)
	const bool ordered = turns >= 1, ordered_decode = turns >= 2;
	if (ordered && stage_order_wait(enc.device(), 0, enc.stream())) return -2;
	if (b->stream.moving && stream_begin_pass(GroupUnits(b))) return -2;      // (in front of the first launch: it rewrites rows of the job tables)
	if (b->host_in && enc.upload_frames(b->host_in, b->host_in_stride, b->host_in_pitch)) return -2;
	if (enc.launch_forward()) return -2;
	for (int g = 0; g < ng; g++) {
		const SampleHeaderInfo h = group_header(b, g);
		if (b->stream.moving) enc.entropy().set_group_plan(b->stream.groups.coded[g]);      // (the header carries the group's own tables)
		if (enc.entropy().set_frame_header(g, h)) return -6;
		if (write_pframe_sample(b->gplan, h.frame_number, b->pframes.data() + (size_t)kPFrameSampleBytes * g, kPFrameSampleBytes) != kPFrameSampleBytes) return -6;
	}
	if (enc.entropy().launch()) return -2;
	if (ordered && stage_order_done(enc.device(), 0, enc.stream())) return -2;
	if (b->decode) {
		GopBatch &dec = *b->gdec;
		if (ordered_decode && stage_order_wait(enc.device(), 1, dec.stream())) return -5;
		dec.batch_entropy().set_producer_events(enc.entropy().headers_event(), enc.entropy().samples_event());
		if (dec.batch_entropy().set_samples_device(enc.entropy().device_samples(), enc.entropy().device_sizes(), enc.entropy().device_offsets())) return -4;
		if (dec.batch_entropy().launch() || dec.launch_inverse(seed, true)) return -5;
		if (ordered_decode && stage_order_done(enc.device(), 1, dec.stream())) return -5;
		if (b->host_out && dec.download_frames(b->host_out, b->host_out_stride, b->host_out_pitch)) return -5;
	}
	if (enc.entropy().download_queue()) return -2;
	b->t_launched = now();
	return 0;
}
// gop_finish: as batch_finish.  Returns the sum of the sizes of the group samples or < 0.
long long gop_finish(cfhd_amd_batch *b)
{
	GopBatch &enc = *b->genc;
	const int ng = b->ngroups();
	if (enc.entropy().download_finish() || enc.wait()) return -2;
	// a stream whose tables move: the rounds behind round 0, as in batch_finish
	if (b->stream.moving) { const int rc = stream_rounds(GroupUnits(b)); if (rc) return rc; }
	// -3 (a sample beyond its buffer: size 0) and -8 (a peak table the device stage cannot write) as for intra batches; -9: a group sample so large that the reference
	// would have coded bands of the frame wavelets as zeros (encoder.c:8332, gop_sample_may_zero_bands) -- what the device stage wrote is not that sample.  All behind
	// the loop: the other samples are complete and keep their sizes.
	bool overflow = false, peaks = false, oversize = false;
	for (int g = 0; g < ng; g++) {
		const size_t n = enc.entropy().sample_bytes(g);
		b->sample_size[2 * g] = n; b->sample_size[2 * g + 1] = n ? (size_t)kPFrameSampleBytes : 0;
		if (!n) { overflow = true; continue; }
		if (enc.entropy().needs_peak_table(g)) peaks = true;
		if (gop_sample_may_zero_bands(b->gplan, n)) oversize = true;
	}
	const double t_enc = now();
	if (b->decode && b->gdec->wait()) return -5;
	if (overflow) return -3;
	if (peaks) return -8;
	if (oversize) return -9;
	if (b->decode && b->gdec->batch_entropy().check()) return -7;
	if (b->decode && b->host_out) {
		std::atomic<int> bad(0);
		parallel_for(b->n, b->n > 8 ? 8 : 1, [&](int i) { if (b->gdec->finish_frame(i, b->host_out + b->host_out_stride * (size_t)i, b->host_out_pitch)) bad.store(1); });
		if (bad.load()) return -5;
	}
	const double t4 = now();
	b->t_fwd = b->t_launched - b->t_launch0; b->t_entropy_enc = t_enc - b->t_launched; b->t_entropy_dec = 0; b->t_inv = t4 - t_enc;
	if (b->stream.on) stream_end_pass(GroupUnits(b));
	b->steps++;
	long long total = 0;
	for (int g = 0; g < ng; g++) total += (long long)b->sample_size[2 * g];
	return total;
}
void gop_drain(cfhd_amd_batch *b) { (void)b->genc->wait(); if (b->decode) (void)b->gdec->wait(); }

// A batch of two-frame groups (cfhd_amd_batch_create_ex with CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP, cfhd_amd_batch_create_groups), or null: never a batch that does
// something else.  coded_lowpass: groups whose w[3] lowpass band is divided and coded in two passes (the 8-bit RGB inputs) are taken too -- cfhd_amd_batch_create_groups;
// cfhd_amd_batch_create_ex keeps refusing them, as the callers that probe with it expect.
// stream: cfhd_amd_batch_create_group_stream's batch -- one encoder's stream, tables that move included (then every group carries tables of its own: stream_rounds).
cfhd_amd_batch *create_group_batch(const FrontEndParams &fp, int width, int height, int nframes, int nthreads, int mode, bool coded_lowpass, bool stream)
{
	const int kind = fp.pixel_kind;
	// whole groups; tables that never move unless the batch is a stream (the group twin of the intra rule below); round trips to the input's own format where a group decodes to it
	if (nframes < 2 || (nframes & 1) || (!fp.gop_static_quantizer && !stream) || (gop_temporal_lowpass_is_coded(fp.gplan) && !coded_lowpass)) return nullptr;
	if (mode != 0 && mode != 1) return nullptr;
	if (mode == 0 && !fp.gop_output_served) return nullptr;
	const char *e = getenv("CFHD_AMD_ENTROPY");
	if (e && strcmp(e, "host") == 0) return nullptr;      // (the host arrangement is the C ABI's)
	cfhd_amd_batch *b = new (std::nothrow) cfhd_amd_batch;
	if (!b) return nullptr;
	b->n = nframes; b->nthreads = nthreads > 0 ? nthreads : 1; b->quality = fp.quality; b->pixel_kind = kind;
	b->color_format = fp.color_format; b->color_space = fp.color_space; b->progressive = fp.progressive;
	b->decode = mode == 0; b->plan = fp.plan; b->gop = true; b->gplan = fp.gplan;
	const int ng = nframes / 2;
	// SampleEncoder.cpp:387 (a group beyond 80 % of it fails its pass: -9).  A stream is one handle's, and the handle keeps two frames' worth for a group
	// (cfhd_api_encoder.inc prepare_group_encoder): the groups the handle can write fit here too -- the bit-rate limiter only trips on groups near one frame's worth
	const size_t cap = ((size_t)width * height * fp.pixel_bytes + 65536) * (stream ? 2 : 1);
	b->sequence_header_size = write_sequence_header(b->gplan, fp.gop_sequence_format, b->sequence_header, sizeof(b->sequence_header));
	b->pframes.assign((size_t)kPFrameSampleBytes * ng, 0);
	b->samples.resize(nframes); b->sample_size.assign(nframes, 0);
	// streams as for intra batches (cfhd_amd_batch_create_ex): one per object unless CFHD_AMD_STREAMS = 1; CFHD_AMD_CHUNK is not read -- one chunk
	const char *sp = getenv("CFHD_AMD_STREAMS"), *hq = getenv("GPU_MAX_HW_QUEUES");
	const int streams = sp && atoi(sp) >= 1 && atoi(sp) <= 3 ? atoi(sp) : (hq && atoi(hq) >= 8 ? 3 : 2);
	struct Lean { Lean() { device_streams_lean(true); } ~Lean() { device_streams_lean(false); } } lean;
	b->genc.reset(new GopBatch);
	if (b->decode) b->gdec.reset(new GopBatch);
	auto encoder = [&] { return !b->genc->prepare(b->gplan, false, kind, false, ng) && !b->genc->prepare_entropy(cap); };
	auto decoder = [&] {
		if (!b->decode) return true;
		// the decoder's plan is the sample's: geometry and scan (its quantizers travel in the sample)
		if (b->gdec->prepare(b->gplan, true, kind, false, ng) || b->gdec->prepare_entropy_decode()) return false;
		// (subband 7 coded in two passes: only where the device group decoder takes it -- dev::DecGroupPlan::two_pass)
		if (gop_temporal_lowpass_is_coded(b->gplan) && !b->gdec->batch_entropy().two_pass_served()) return false;
		// the outputs that convert to RGB take the matrix of the colour space the group samples are tagged with (frame 1 of every group: 709, GopBatch::fill_jobs)
		b->gdec->set_color_matrix((fp.color_space & 3) == 1 ? 2 : 0);
		return true;
	};
	bool ok;
	if (streams == 1) { StreamScope scope; ok = encoder() && decoder(); if (scope.stream()) b->shared_streams.push_back(scope.stream()); }
	else if (streams == 2) {
		{ StreamScope scope; ok = encoder(); if (scope.stream()) b->shared_streams.push_back(scope.stream()); }
		if (ok) { StreamScope scope; ok = decoder(); if (scope.stream()) b->shared_streams.push_back(scope.stream()); }
	} else ok = encoder() && decoder();
	if (!ok || b->sequence_header_size != kSequenceHeaderBytes) { delete b; return nullptr; }
	b->genc->set_timed(true);
	if (b->decode) b->gdec->set_timed(true);
	if (stream) {
		cfhd_amd_batch::Stream &s = b->stream;
		s.on = true; s.moving = !fp.gop_static_quantizer; s.derive_quality = fp.derive_quality;
		s.carried = fp.gqstate; s.groups.carried_plan = fp.gplan; s.carried_bytes = 0; s.next = fp.gqstate;
		if (s.moving) { s.groups.coded.assign((size_t)ng, fp.gplan); s.before.assign((size_t)ng, fp.gqstate); }
	}
	return b;
}
}

extern "C" {
long long cfhd_amd_batch_wait(cfhd_amd_batch *b);

// width x height frames of `pixel_format` encoded as `encoded_format` with `encoding_flags` (the CFHD_PrepareToEncode arguments: YUY2 / 2vuy ->
// 4:2:2, optionally interlaced; RG48 -> RGB 4:4:4; b64a -> RGBA 4:4:4:4; BYR4 -> Bayer).  mode 0: encode + decode back to the same pixel
// format; mode 1: encode only (the only mode for BYR4 / BYR5 and the Avid 4:2:2 layouts, which no decoder output has).
cfhd_amd_batch *cfhd_amd_batch_create_ex(int width, int height, uint32_t pixel_format, int encoded_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode)
{
	CallerDevice caller_device;
	FrontEndParams fp;
	if (nframes < 1 || front_end_params(width, height, pixel_format, encoded_format, encoding_flags, quality, &fp)) return nullptr;
	// A batch encodes its frames in one launch with one set of quantizer tables.  Qualities whose tables follow the size of the previous sample
	// (FILMSCAN2/3, LOW..HIGH up to 1080p: encoder.c:3414 -> quantize.c:2869) need frame i's sample before frame i + 1 can start -- those
	// sequences go through CFHD_EncodeSample, which applies the feedback per frame, or through cfhd_amd_batch_create_stream, which codes a pass on a guess of
	// every frame's tables and codes the frames behind a wrong guess again; here they are refused instead of encoded differently (callers probe with this entry).
	if (fp.gop) return create_group_batch(fp, width, height, nframes, nthreads, mode, false, false);
	if (!fp.static_quantizer) return nullptr;
	return create_intra_batch(fp, width, height, nframes, nthreads, mode, false);
}

// One encoder's stream on the frame queue (include/cfhd_amd.h): every quality word CFHD_PrepareToEncode takes for intra frames.  A word whose tables never move makes
// exactly cfhd_amd_batch_create_ex's batch; one whose tables follow the sizes makes the same batch with tables per frame and the rounds of stream_rounds behind round 0.
cfhd_amd_batch *cfhd_amd_batch_create_stream(int width, int height, uint32_t pixel_format, int encoded_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode)
{
	CallerDevice caller_device;
	FrontEndParams fp;
	auto refuse = [](const char *text) { device_set_last_error(text); return (cfhd_amd_batch *)nullptr; };
	if (nframes < 1) return refuse("cfhd_amd_batch_create_stream: a batch has at least one frame");
	if (mode != 0 && mode != 1) return refuse("cfhd_amd_batch_create_stream: mode is 0 (round trip) or 1 (encode only)");
	if (encoding_flags & (1u << 1)) return refuse("cfhd_amd_batch_create_stream: two-frame groups go through cfhd_amd_batch_create_groups (tables that stand still) or cfhd_amd_batch_create_group_stream (any tables)");
	if (front_end_params(width, height, pixel_format, encoded_format, encoding_flags, quality, &fp)) return refuse("cfhd_amd_batch_create_stream: arguments CFHD_PrepareToEncode refuses");
	const char *e = getenv("CFHD_AMD_ENTROPY");
	if (e && strcmp(e, "host") == 0) return refuse("cfhd_amd_batch_create_stream: CFHD_AMD_ENTROPY=host keeps the entropy stage on the host; a stream is coded on the device");
	device_set_last_error("");
	cfhd_amd_batch *b = create_intra_batch(fp, width, height, nframes, nthreads, mode, true);
	if (!b && !*device_last_error()) device_set_last_error("cfhd_amd_batch_create_stream: cfhd_amd_batch_create_ex refuses this input, mode or arrangement");
	return b;
}
}

extern "C" {
// Bayer mosaics on the frame queue (include/cfhd_amd.h): BYR4 / BYR5 -> Bayer samples; mode 1 is exactly cfhd_amd_batch_create_ex's batch, mode 0 -- BYR4 -- adds the
// decode back to the mosaic.  The tables stand still (as cfhd_amd_batch_create_ex: a Bayer stream with rate feedback is not built).
cfhd_amd_batch *cfhd_amd_batch_create_bayer(int width, int height, uint32_t pixel_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode)
{
	CallerDevice caller_device;
	FrontEndParams fp;
	auto refuse = [](const char *text) { device_set_last_error(text); return (cfhd_amd_batch *)nullptr; };
	if (nframes < 1) return refuse("cfhd_amd_batch_create_bayer: a batch has at least one frame");
	if (mode != 0 && mode != 1) return refuse("cfhd_amd_batch_create_bayer: mode is 0 (round trip) or 1 (encode only)");
	if (pixel_format != 0x42595234u /* 'BYR4' */ && pixel_format != 0x42595235u /* 'BYR5' */) return refuse("cfhd_amd_batch_create_bayer: the input is a Bayer mosaic, BYR4 or BYR5");
	if (front_end_params(width, height, pixel_format, 3 /* CFHD_ENCODED_FORMAT_BAYER */, encoding_flags, quality, &fp) || fp.gop)
		return refuse("cfhd_amd_batch_create_bayer: arguments CFHD_PrepareToEncode refuses");
	if (fp.pixel_kind == PIX_BYR5 && mode == 0) return refuse("cfhd_amd_batch_create_bayer: BYR5 is no decoder output; mode 1 encodes only");
	if (!fp.static_quantizer) return refuse("cfhd_amd_batch_create_bayer: the tables of this quality follow the sample sizes (a Bayer stream is not built: CFHD_EncodeSample encodes such a sequence)");
	device_set_last_error("");
	cfhd_amd_batch *b = create_intra_batch(fp, width, height, nframes, nthreads, mode, false, true);
	if (!b && !*device_last_error()) device_set_last_error("cfhd_amd_batch_create_bayer: cfhd_amd_batch_create_ex refuses this arrangement");
	return b;
}
}

namespace {
// An intra batch: cfhd_amd_batch_create_ex's (tables that stand still) and, with stream, cfhd_amd_batch_create_stream's (any tables).  bayer_round_trip:
// cfhd_amd_batch_create_bayer's -- the same batch, whose mode 0 decodes BYR4 back to the mosaic (large launches by the fused last level, DecodeBatch::set_bayer_strips).
cfhd_amd_batch *create_intra_batch(const FrontEndParams &fp, int width, int height, int nframes, int nthreads, int mode, bool stream, bool bayer_round_trip)
{
	const int kind = fp.pixel_kind;
	const bool yuv = kind == PIX_YUY2 || kind == PIX_2VUY;
	cfhd_amd_batch *b = new (std::nothrow) cfhd_amd_batch;
	if (!b) return nullptr;
	b->n = nframes; b->nthreads = nthreads > 0 ? nthreads : 1; b->quality = fp.quality; b->pixel_kind = kind;
	b->color_format = fp.color_format; b->color_space = fp.color_space; b->progressive = fp.progressive;
	b->decode = mode == 0;
	b->plan = fp.plan;
	if (b->decode && ((kind == PIX_BYR4 && !bayer_round_trip) || kind == PIX_BYR5 || is_avid_422(kind))) { delete b; return nullptr; }      // (no decoder output of these layouts; BYR4: cfhd_amd_batch_create_bayer)
	const char *e = getenv("CFHD_AMD_ENTROPY");
	b->gpu_entropy = !(e && strcmp(e, "host") == 0);
	if (!b->gpu_entropy && (!yuv || !b->progressive || !b->decode)) { delete b; return nullptr; }      // the host-entropy arrangement is kept for the headline workload only
	const char *ho = getenv("CFHD_AMD_HANDOFF");
	b->device_handoff = b->gpu_entropy && !(ho && strcmp(ho, "host") == 0);
	const char *cs = getenv("CFHD_AMD_CHUNK");
	int chunk = cs ? atoi(cs) : 0;                     // 0 = whole batch in one chunk (measured fastest: launches are already batch-wide)
	if (chunk <= 0 || !b->gpu_entropy) chunk = nframes;
	const size_t cap = (size_t)width * height * fp.pixel_bytes + 65536;        // SampleEncoder.cpp:387
	// Streams of a pass.  The runtime deals its hardware queues (GPU_MAX_HW_QUEUES, 4 unless the application's environment says otherwise) to a process's streams in the
	// order of their creation, and streams on one queue take turns (cfhd_entropy_gpu.h device_stream_create).  Measured with four passes in flight (profiles/r06_d_*):
	//   4 queues:  one stream per pass 55.5 k fps, two (encoder | decoder) 57.9 k, three (transforms | level-1 count | decoder) 56.9 k   [round 5: four, one unused: 50.4-50.8 k]
	//   16 queues: 45.3 k / 59.8 k / 61.2 k
	// so a pass takes two streams unless the environment gives the process eight queues or more -- read, never set here.  CFHD_AMD_STREAMS=1|2|3 overrides (A/B).
	const char *sp = getenv("CFHD_AMD_STREAMS"), *hq = getenv("GPU_MAX_HW_QUEUES");
	const int streams = sp && atoi(sp) >= 1 && atoi(sp) <= 3 ? atoi(sp) : (hq && atoi(hq) >= 8 ? 3 : 2);
	struct Lean { Lean() { device_streams_lean(true); } ~Lean() { device_streams_lean(false); } } lean;      // (a batch creates only the streams it launches on)
	for (int first = 0; first < nframes; first += chunk) {
		std::unique_ptr<cfhd_amd_chunk> c(new cfhd_amd_chunk);
		c->first = first; c->n = nframes - first < chunk ? nframes - first : chunk;
		bool ok = true;
		auto encoder = [&] { return !c->enc.prepare(b->plan, c->n) && !(b->gpu_entropy && c->enc.prepare_entropy(cap)); };
		auto decoder = [&] { if (!b->decode) return true; c->dec.set_interlaced(!b->progressive); c->dec.set_bayer_strips(bayer_round_trip); return !c->dec.prepare(b->plan, c->n, kind) && !(b->gpu_entropy && c->dec.prepare_entropy(cap)); };
		if (streams == 1) { StreamScope scope; ok = encoder() && decoder(); if (scope.stream()) b->shared_streams.push_back(scope.stream()); }
		else if (streams == 2) {
			// (CFHD_AMD_STREAM_ORDER=alt, A/B: every second batch of the process creates its decoder's stream first -- with four queues dealt in creation order the encoder of
			// one pass then shares its queue with the decoder of another instead of with another encoder)
			static std::atomic<unsigned> created(0);
			static const bool alternate = [] { const char *e = getenv("CFHD_AMD_STREAM_ORDER"); return e && strcmp(e, "alt") == 0; }();
			void *dec_stream = nullptr;
			if (alternate && b->decode && (created.fetch_add(1) & 1u)) { StreamScope scope; void *x = nullptr; if (device_stream_create(&x) == 0) dec_stream = x; }
			{ StreamScope scope; ok = encoder(); if (scope.stream()) b->shared_streams.push_back(scope.stream()); }
			if (ok) { StreamScope scope(dec_stream); ok = decoder(); if (scope.stream()) b->shared_streams.push_back(scope.stream()); }
			else if (dec_stream) b->shared_streams.push_back(dec_stream);
		} else ok = encoder() && decoder();
		b->chunks.push_back(std::move(c));                // (also when it failed: the batch's destructor releases what was prepared, then the scopes' streams)
		if (!ok) { delete b; return nullptr; }
	}
	b->samples.resize(nframes); b->sample_size.assign(nframes, 0);
	if (!b->gpu_entropy) for (auto &s : b->samples) s.resize(cap);
	if (stream) {
		cfhd_amd_batch::Stream &s = b->stream;
		s.on = true; s.moving = !fp.static_quantizer; s.derive_quality = fp.derive_quality;
		s.carried = fp.qstate; s.frames.carried_plan = fp.plan; s.carried_bytes = 0; s.next = fp.qstate;
		if (s.moving) {
			// the rounds sit between the two halves of the default pass: nothing else has them
			if (!(b->gpu_entropy && b->device_handoff && b->chunks.size() == 1)) {
				delete b;
				device_set_last_error("cfhd_amd_batch_create_stream: tables that follow the sample sizes need the default arrangement (no CFHD_AMD_HANDOFF=host, no CFHD_AMD_CHUNK)");
				return nullptr;
			}
			s.frames.coded.assign((size_t)nframes, fp.plan); s.before.assign((size_t)nframes, fp.qstate);
		}
	}
	return b;
}
}

extern "C" {

// Two-frame groups from any input cfhd_amd_batch_create_ex takes with encoded format 0 and CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP (implied here) -- the same batch, byte
// for byte -- and from RG24 / BGRA / BGRa, whose subband 7 is divided and coded in two passes (k_ent_split_two_pass; mode 0: k_dec_band_two_pass).
cfhd_amd_batch *cfhd_amd_batch_create_groups(int width, int height, uint32_t pixel_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode)
{
	CallerDevice caller_device;
	FrontEndParams fp;
	if (nframes < 1 || front_end_params(width, height, pixel_format, 0, encoding_flags | (1u << 1) /* CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP */, quality, &fp) || !fp.gop) return nullptr;
	return create_group_batch(fp, width, height, nframes, nthreads, mode, true, false);
}

// One group encoder's stream on the frame queue (include/cfhd_amd.h): every quality word CFHD_PrepareToEncode takes for groups.  A word whose group tables never move
// makes exactly cfhd_amd_batch_create_groups' batch; one whose tables follow the key samples makes the same batch with tables per group and the rounds of
// stream_rounds behind round 0.
cfhd_amd_batch *cfhd_amd_batch_create_group_stream(int width, int height, uint32_t pixel_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode)
{
	CallerDevice caller_device;
	FrontEndParams fp;
	auto refuse = [](const char *text) { device_set_last_error(text); return (cfhd_amd_batch *)nullptr; };
	if (nframes < 2 || (nframes & 1)) return refuse("cfhd_amd_batch_create_group_stream: a batch holds whole two-frame groups, at least one");
	if (mode != 0 && mode != 1) return refuse("cfhd_amd_batch_create_group_stream: mode is 0 (round trip) or 1 (encode only)");
	if (front_end_params(width, height, pixel_format, 0, encoding_flags | (1u << 1) /* CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP */, quality, &fp) || !fp.gop)
		return refuse("cfhd_amd_batch_create_group_stream: arguments CFHD_PrepareToEncode refuses for two-frame groups");
	const char *e = getenv("CFHD_AMD_ENTROPY");
	if (e && strcmp(e, "host") == 0) return refuse("cfhd_amd_batch_create_group_stream: CFHD_AMD_ENTROPY=host keeps the entropy stage on the host; a stream is coded on the device");
	const char *ho = getenv("CFHD_AMD_HANDOFF");
	if (!fp.gop_static_quantizer && ho && strcmp(ho, "host") == 0)
		return refuse("cfhd_amd_batch_create_group_stream: tables that follow the sample sizes need the default arrangement (no CFHD_AMD_HANDOFF=host)");
	if (mode == 0 && !fp.gop_output_served) return refuse("cfhd_amd_batch_create_group_stream: a group does not decode to this input's format; mode 1 encodes only");
	device_set_last_error("");
	cfhd_amd_batch *b = create_group_batch(fp, width, height, nframes, nthreads, mode, true, true);
	if (!b && !*device_last_error()) device_set_last_error("cfhd_amd_batch_create_group_stream: cfhd_amd_batch_create_groups refuses this input, mode or arrangement");
	return b;
}

cfhd_amd_batch *cfhd_amd_batch_create(int width, int height, uint32_t pixel_format, int quality, int nframes, int nthreads)
{
	return cfhd_amd_batch_create_ex(width, height, pixel_format == 0x32767579u /* '2vuy' */ ? pixel_format : 0x59555932u /* 'YUY2' */, 0, 0, quality, nframes, nthreads, 0);
}

void cfhd_amd_batch_destroy(cfhd_amd_batch *b) { CallerDevice caller_device; if (b && b->in_flight) (void)cfhd_amd_batch_wait(b); delete b; }

// Puts frame i into HBM (outside the timed region of the benchmark).
int cfhd_amd_batch_upload(cfhd_amd_batch *b, int i, const void *frame, int pitch)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || i < 0 || i >= b->n) return -1;
	if (b->gop) { const int rc = b->genc->upload_frame(i, frame, pitch); return rc ? rc : b->genc->wait(); }
	int l; cfhd_amd_chunk &c = b->chunk_of(i, &l);
	int rc = c.enc.upload_frame(l, frame, pitch);
	if (rc) return rc;
	return c.enc.wait();
}

// Frame i from HBM on the batch's device: queued on the stream the pass runs on, no host wait (the source is borrowed until the next wait / roundtrip returns).
int cfhd_amd_batch_upload_device(cfhd_amd_batch *b, int i, const void *d_frame, int pitch)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || i < 0 || i >= b->n || !d_frame) return -1;
	if (b->gop) return b->genc->upload_frame_device(i, d_frame, pitch);
	int l; cfhd_amd_chunk &c = b->chunk_of(i, &l);
	return c.enc.upload_frame_device(l, d_frame, pitch);
}

// Frames first_frame .. first_frame + count - 1 of an RG48 batch from planar R, G, B tensors -- of a BYR4 batch from the four planes of a mosaic, k_enc_collect_bayer; of
// a YUY2, 2vuy or YU64 batch from a luma and two chroma planes, k_enc_collect_yuv422; of a b64a, BGRA or BGRa batch from four planes R, G, B, A, k_enc_collect_rgba -- in HBM on the batch's device: one k_enc_collect launch on the stream the
// pass runs on (an intra batch cut into chunks: one per chunk the run touches, on that chunk's stream), no staging, no host wait.  The gates that need the geometry
// are the encoder objects' (collect_planar_frames, cfhd_device.hip); they depend on nothing a chunk has of its own, so a run is refused before any of it is launched.
int cfhd_amd_batch_upload_device_planar(cfhd_amd_batch *b, int first_frame, int count, const void *d_frames, size_t frame_stride, int row_pitch, int layout)
{
	CallerDevice caller_device;
	if (!b) { device_set_last_error("cfhd_amd_batch_upload_device_planar: no batch"); return -1; }
	if (b->in_flight) { device_set_last_error("cfhd_amd_batch_upload_device_planar: a pass is in flight"); return -1; }
	if (count < 1 || first_frame < 0 || first_frame > b->n - count) { device_set_last_error("cfhd_amd_batch_upload_device_planar: the run of frames leaves the batch"); return -1; }
	if (b->gop) return b->genc->upload_frames_device_planar(first_frame, count, d_frames, frame_stride, row_pitch, layout);
	for (auto &c : b->chunks) {
		const int lo = first_frame > c->first ? first_frame : c->first, hi = first_frame + count < c->first + c->n ? first_frame + count : c->first + c->n;
		if (lo >= hi) continue;
		const uint8_t *src = d_frames ? (const uint8_t *)d_frames + frame_stride * (size_t)(lo - first_frame) : nullptr;
		const int rc = c->enc.upload_frames_device_planar(lo - c->first, hi - lo, src, frame_stride, row_pitch, layout);
		if (rc) return rc;
	}
	return 0;
}

// Frame i as the batch holds it, in its packed input format (the twin of cfhd_amd_batch_download_output for the input side): waits for the stream the uploads run on.
int cfhd_amd_batch_download_frame(cfhd_amd_batch *b, int i, void *out, int pitch)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || i < 0 || i >= b->n || !out) return -1;
	if (b->gop) return b->genc->download_input_frame(i, out, pitch);
	int l; cfhd_amd_chunk &c = b->chunk_of(i, &l);
	return c.enc.download_input_frame(l, out, pitch);
}

// One step of the hot path over the whole batch.  Returns the total number of sample bytes, or < 0.
static long long cfhd_amd_batch_roundtrip_locked(cfhd_amd_batch *b);
// (A batch with a pass in flight -- cfhd_amd_batch_submit without its _wait -- refuses every entry point that would touch its streams, job tables or pinned buffers: -1.)
long long cfhd_amd_batch_roundtrip(cfhd_amd_batch *b)
{
	if (!b || b->in_flight) return -1;
	return cfhd_amd_batch_roundtrip_locked(b);
}
static long long cfhd_amd_batch_roundtrip_locked(cfhd_amd_batch *b)
{
	CallerDevice caller_device;
	if (b->gop) {
		const int rc = gop_launch(b);
		if (rc) { gop_drain(b); return rc; }
		const long long total = gop_finish(b);
		if (total < 0) gop_drain(b);
		return total;
	}
	const FramePlan &plan = b->plan;
	double t0 = now(), t1, t2, t3;
	std::atomic<int> bad(0);
	const uint32_t base_number = b->steps * (uint32_t)b->n;
	// every frame gets the metadata CFHD_EncodeSample would give it: GUID, encode date / time, a timecode and a unique frame number that advance per frame
	b->frame_meta.resize(b->n);
	bool meta_ready = false;
	auto prepare_meta = [&] { if (meta_ready) return; meta_ready = true; for (int i = 0; i < b->n; i++) { b->meta.handle(); b->frame_meta[i] = b->meta.global; meta_remove_hidden(b->frame_meta[i]); } };
	auto header = [&](int i) { SampleHeaderInfo h = { base_number + (uint32_t)i + 1, b->color_format, b->color_space, b->quality, b->progressive, b->frame_meta[i].data(), b->frame_meta[i].size(), nullptr, 0 }; return h; };
	const uint32_t seed = 0xA511E9B3u * (b->steps + 1);
	if (b->gpu_entropy && b->device_handoff && b->chunks.size() == 1) {
		const int rc = batch_launch(b);
		if (rc) return rc;
		return batch_finish(b);
	}
	for (auto &c : b->chunks) c->enc.collect_begin_pass();      // (as in batch_launch)
	if (b->gpu_entropy && b->device_handoff) {
		// Samples stay in HBM between the encoder and the decoder: the decoder's stream waits for the encoder's kernels, parses
		// the samples on the GPU and decodes, while the finished samples travel to the host (the encoder's product) on the
		// encoder's stream beside it.
		// Every chunk is driven by its own host thread from its first launch to its last wait, on its own streams.  (Queued from one thread, four
		// chunks of 128 ran at 36.5 k fps where one chunk of 512 runs at 46 k: the chunks did not overlap.  Four threads with 128 frames each: +10 %
		// over the single chunk -- the VALU-bound entropy kernels of one chunk run beside the HBM-bound transforms of another.  gpurun_out/r03i, r03j.)
		prepare_meta();
		std::atomic<int> err(0);
		std::vector<double> t_sub(b->chunks.size(), 0.0), t_enc(b->chunks.size(), 0.0);
		parallel_for((int)b->chunks.size(), (int)b->chunks.size(), [&](int k) {
			cfhd_amd_chunk *c = b->chunks[k].get();
			auto fail = [&](int code) { int z = 0; err.compare_exchange_strong(z, code); };
			// the transform kernels start first: the host serialises the sample headers (0.5 ms per 256) while they run
			if (c->enc.launch_forward(false)) return fail(-2);      // (nothing but the entropy stage reads these coefficients)
			for (int l = 0; l < c->n; l++) if (c->enc.entropy().set_frame_header(l, header(c->first + l))) return fail(-6);
			if (c->enc.entropy().launch()) return fail(-2);
			if (b->decode) {
				// the parser only needs the headers and size fields (k_ent_layout): it runs beside k_ent_emit, the band decoder waits for the payloads
				c->dec.entropy().set_producer_events(c->enc.entropy().headers_event(), c->enc.entropy().samples_event());
				if (c->dec.entropy().set_samples_device(c->enc.entropy().device_samples(), 0, c->enc.entropy().device_sizes(), c->enc.entropy().device_offsets())) return fail(-4);
				if (c->dec.launch_entropy() || c->dec.launch_inverse(seed + (uint32_t)c->first)) return fail(-5);
			}
			t_sub[k] = now();
			if (c->enc.entropy().download() || c->enc.wait()) return fail(-2);
			for (int l = 0; l < c->n; l++) {
				size_t n = c->enc.entropy().sample_bytes(l); b->sample_size[c->first + l] = n; if (!n) { fail(-3); continue; }      // (the other frames keep their samples and sizes)
				if (c->enc.entropy().needs_peak_table(l)) fail(-8);             // a band with more peak values than the entropy stage's positions hold (two million): only CFHD_EncodeSample writes such a sample (host writer)
			}
			t_enc[k] = now();
			if (b->decode) { if (c->dec.wait()) return fail(-5); if (c->dec.entropy().check()) return fail(-7); }
		});
		if (err.load()) return err.load();
		t1 = t0; t2 = t0;
		for (size_t k = 0; k < b->chunks.size(); k++) { if (t_sub[k] > t1) t1 = t_sub[k]; if (t_enc[k] > t2) t2 = t_enc[k]; }
		if (t2 < t1) t2 = t1;
		t3 = t2;
	} else if (b->gpu_entropy) {
		// 1. every chunk: forward transform + entropy coding, queued on the chunk's own stream
		prepare_meta();
		for (auto &c : b->chunks) {
			for (int l = 0; l < c->n; l++) if (c->enc.entropy().set_frame_header(l, header(c->first + l))) return -6;
			if (c->enc.launch_forward(false) || c->enc.entropy().launch()) return -2;
		}
		t1 = now();
		// 2. as each chunk's samples arrive on the host (the encoder's product), hand them to the decoder and queue its work
		double wait_s = 0, stage_s = 0;
		int pass_err = 0;
		for (auto &c : b->chunks) {
			double a = now();
			if (c->enc.entropy().download() || c->enc.wait()) return -2;
			// (an oversize frame, -3, or one that needs the host writer's peak table, -8, fails the pass behind the loops, as in batch_finish: every frame's size is recorded,
			// the chunk's pictures are not decoded, the decoders already at work drain)
			bool undecodable = false;
			for (int l = 0; l < c->n; l++) {
				size_t n = c->enc.entropy().sample_bytes(l); b->sample_size[c->first + l] = n;
				if (!n) { if (!pass_err) pass_err = -3; undecodable = true; continue; }
				if (c->enc.entropy().needs_peak_table(l)) { if (!pass_err) pass_err = -8; undecodable = true; }
			}
			double m = now();
			if (!b->decode || undecodable) { wait_s += m - a; continue; }
			cfhd_amd_chunk *cp = c.get();
			parallel_for(c->n, b->nthreads < 16 ? b->nthreads : 16, [&, cp](int l) {
				if (cp->dec.entropy().set_sample_host(l, cp->enc.entropy().host_sample(l), b->sample_size[cp->first + l])) bad++; });
			if (bad) return -4;
			if (c->dec.launch_entropy() || c->dec.launch_inverse(seed + (uint32_t)c->first)) return -5;
			wait_s += m - a; stage_s += now() - m;
		}
		t2 = t1 + wait_s; t3 = t2 + stage_s;
		// 3. drain
		if (b->decode) for (auto &c : b->chunks) { if (c->dec.wait()) return -5; if (!pass_err && c->dec.entropy().check()) return -7; }
		if (pass_err) return pass_err;
	} else {
		cfhd_amd_chunk &c = *b->chunks[0];
		prepare_meta();
		if (c.enc.launch_forward() || c.enc.download_coeffs() || c.enc.wait()) return -2;
		t1 = now();
		parallel_for(b->n, b->nthreads, [&](int i) {
			SampleHeaderInfo hdr = header(i);
			BandSource src; src.coeffs = c.enc.host_coeffs(i);
			size_t n = write_sample(plan, hdr, src, b->samples[i].data(), b->samples[i].size());
			if (!n) bad++;
			b->sample_size[i] = n;
		});
		t2 = now();
		if (bad) return -3;
		parallel_for(b->n, b->nthreads, [&](int i) {
			const uint8_t *s = b->samples[i].data();
			ParsedSample ps;
			if (parse_sample(s, b->sample_size[i], &ps) != 0) { bad++; return; }
			c.dec.clear_host_coeffs(i);
			int16_t *coeffs = c.dec.host_coeffs(i);
			for (int ch = 0; ch < plan.num_channels; ch++) {
				const ParsedBand &lp = ps.lowpass[ch];
				const BandDesc &ll = plan.ch[ch].band[2][0];
				const int bias = lowpass_bias(plan.precision, ll.width, b->pixel_kind, ch);
				for (int r = 0; r < ll.height; r++) {
					const uint8_t *p = s + lp.offset + (size_t)r * ll.width * 2;
					int16_t *dst = coeffs + ll.offset + (size_t)r * ll.pitch;
					for (int x = 0; x < ll.width; x++) { int v = (int16_t)((p[2 * x] << 8) | p[2 * x + 1]); v += bias; dst[x] = (int16_t)(v > 0x7fff ? 0x7fff : v); }
				}
				for (int lv = 0; lv < kNumLevels; lv++)
					for (int k = 1; k < 4; k++) {
						const ParsedBand &pb = ps.high[ch][lv][k];
						const BandDesc &bd = plan.ch[ch].band[lv][k];
						if (!pb.present || vlc_decode_band(s + pb.offset, pb.bytes, bd.width, bd.height, bd.pitch, pb.quant, pb.codebook, coeffs + bd.offset)) { bad++; return; }
					}
			}
		});
		t3 = now();
		if (bad) return -4;
		if (c.dec.upload_coeffs() || c.dec.launch_inverse(seed) || c.dec.wait()) return -5;
	}
	double t4 = now();
	b->t_fwd = t1 - t0; b->t_entropy_enc = t2 - t1; b->t_entropy_dec = t3 - t2; b->t_inv = t4 - t3;
	if (b->stream.on) stream_end_pass(FrameUnits(b));   // (a stream whose tables stand still, in one of the other arrangements)
	b->steps++;
	long long total = 0;
	for (int i = 0; i < b->n; i++) total += (long long)b->sample_size[i];
	return total;
}

// The streaming form (north_star: "the EncoderPool / AsyncEncoder thread pool is replaced by a HIP-stream frame queue"; semantics of the reference's queue:
// EncoderSDK/EncoderPool.cpp:239-380 -- submit returns at once, results are collected in submission order).  A batch object is one slot of the queue: submit starts
// its pass (all launches asynchronous on the batch's own streams, driven by a thread of its own), wait collects it.  Several batch objects in flight overlap: while
// one pass is in its instruction-bound entropy kernels another's bandwidth-bound transforms run beside them, which a single synchronous pass cannot have
// (tools/dual_batch.py).  The caller keeps FIFO order by waiting in the order it submitted.
int cfhd_amd_batch_submit(cfhd_amd_batch *b)
{
	CallerDevice caller_device;
	if (!b || b->in_flight) return -1;
	b->pending = -1;
	CountedSubmit pass(b);
	// CFHD_AMD_QUEUE=thread: (A/B) the blocking pass on a thread of its own for the default arrangement too, as in round 4.  (Also measured: the launches of a queued
	// pass -- 2-3 ms of host time with the serialising of 512 sample headers -- on a short-lived thread instead of the caller's: no difference on any line, profiles/r05_q_*.)
	static const bool threaded = [] { const char *e = getenv("CFHD_AMD_QUEUE"); return e && strcmp(e, "thread") == 0; }();
	if (b->gop && !threaded) {
		b->genc->entropy().set_speculative_download(true);
		const int rc = gop_launch(b);                      // the whole pass is on the batch's streams when this returns; nothing waits
		if (rc) { gop_drain(b); b->genc->entropy().set_speculative_download(false); return rc; }
		return pass.keep(true);
	}
	if (b->gpu_entropy && b->device_handoff && b->chunks.size() == 1 && !threaded) {
		b->chunks[0]->enc.entropy().set_speculative_download(true);
		const int rc = batch_launch(b);                   // the whole pass is on the batch's streams when this returns; nothing waits
		if (rc) {                                         // a launch that failed midway: drain what it queued, leave the batch idle (advisor, round 5)
			(void)b->chunks[0]->enc.wait(); if (b->decode) (void)b->chunks[0]->dec.wait();
			b->chunks[0]->enc.entropy().set_speculative_download(false);
			return rc;
		}
		return pass.keep(true);
	}
	pass.keep(false);
	b->worker = std::thread([b] { b->pending = cfhd_amd_batch_roundtrip_locked(b); });
	return 0;
}

// The frame queue fed from host memory (what EncoderSDK/EncoderPool.cpp:239-295 is to the reference: frames in, samples out, nothing resident): the pass copies its n frames
// from `frames` (frame i at frames + i * frame_stride, rows `pitch` bytes apart) into HBM on its own stream, runs, and copies the n decoded pictures to `pictures` (likewise;
// null: none) -- all queued behind one another, so that with several batches in flight the copies of one pass run beside the kernels of the others.  Both buffers are
// borrowed until cfhd_amd_batch_wait returns; buffers registered with cfhd_amd_register_host_buffer are DMA sources / targets as they are (one copy each way when the frames
// lie back to back at the batch's own pitch), plain buffers are staged through pinned memory by the calling thread.  The samples arrive as for cfhd_amd_batch_submit.
int cfhd_amd_batch_submit_host(cfhd_amd_batch *b, const void *frames, size_t frame_stride, int pitch, void *pictures, size_t picture_stride, int picture_pitch)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || !frames || pitch <= 0 || (pictures && (!b->decode || picture_pitch <= 0))) return -1;
	if (!b->gop && !(b->gpu_entropy && b->device_handoff && b->chunks.size() == 1)) return -9;      // (the arrangements with host work in the middle of a pass are not queued: cfhd_amd_batch_upload + _submit)
	b->pending = -1;
	b->host_in = (const uint8_t *)frames; b->host_in_stride = frame_stride; b->host_in_pitch = pitch;
	b->host_out = (uint8_t *)pictures; b->host_out_stride = picture_stride; b->host_out_pitch = picture_pitch;
	CountedSubmit pass(b);
	if (b->gop) {
		b->genc->entropy().set_speculative_download(true);
		const int rc = gop_launch(b);
		if (rc) { b->host_in = nullptr; b->host_out = nullptr; gop_drain(b); b->genc->entropy().set_speculative_download(false); return rc; }
		return pass.keep(true);
	}
	b->chunks[0]->enc.entropy().set_speculative_download(true);
	const int rc = batch_launch(b);
	if (rc) { b->host_in = nullptr; b->host_out = nullptr; (void)b->chunks[0]->enc.wait(); if (b->decode) (void)b->chunks[0]->dec.wait(); b->chunks[0]->enc.entropy().set_speculative_download(false); return rc; }
	return pass.keep(true);
}

long long cfhd_amd_batch_wait(cfhd_amd_batch *b)
{
	CallerDevice caller_device;
	if (!b || !b->in_flight) return -1;
	if (b->queued && b->gop) {
		b->pending = gop_finish(b);
		if (b->pending < 0) gop_drain(b);
		b->host_in = nullptr; b->host_out = nullptr;
	} else if (b->queued) {
		b->pending = batch_finish(b);
		if (b->pending < 0) { cfhd_amd_chunk *c = b->chunks[0].get(); (void)c->enc.wait(); if (b->decode) (void)c->dec.wait(); }      // an error exit must not leave work on the batch's streams (advisor, round 5)
		b->host_in = nullptr; b->host_out = nullptr;
	}
	else b->worker.join();
	pass_counted(b, false);
	b->in_flight = false; b->queued = false;
	return b->pending;
}

// which: 0..2 forward level launches (0 = k_fwd_yuv422), 3..5 inverse level launches (3 = k_inv_yuv422), 6 forward total, 7 inverse total,
// 8..11 k_ent_count / k_ent_scan / k_ent_layout / k_ent_emit, 12..14 k_dec_parse / band decoder (all its kernels) / k_dec_lowpass,
// 15..17 k_dec_index / k_dec_chain / k_dec_tiles, 18 the level-1 part of k_ent_count on its own stream (then 8 is the rest of it; 0 when the count is one
// launch), 19 k_dec_plan (the single workgroup that numbers the chunks in front of k_dec_index) (ms, HIP events on the launch streams),
// 20 -- both kinds of batch -- the k_enc_collect launches that fed the pass (cfhd_amd_batch_upload_device_planar; 0 when none did)
// Batches of two-frame groups: 0 level 1 of all frames, 1 the temporal step + the two middle wavelets (k_gop_temporal_fwd, k_fwd_plane over 6 jobs a group), 2 the
// top wavelet (k_fwd_plane over 3); 3 the last level of all frames + the output conversion, 4 the two middle wavelets + the temporal step (k_inv_plane,
// k_gop_temporal_inv), 5 the top wavelet (k_inv_plane); 6 / 7 the sums of 0..2 / 3..5; 8..11 as above; 12 k_dec_parse_group, 13 the band decoder (k_dec_bands_par of
// both code sets + k_dec_undiff), 14 k_dec_lowpass; 15..19: 0 (no chunk-indexed decoder, no split count).  The slots are in launch order 0, 1, 2, 5, 4, 3 as for intra batches.
float cfhd_amd_batch_kernel_ms(cfhd_amd_batch *b, int which)
{
	if (!b || b->in_flight) return 0;
	if (which == 20) { float ms = b->gop ? b->genc->collect_ms() : 0.0f; for (auto &c : b->chunks) ms += c->enc.collect_ms(); return ms; }
	if (b->gop) {
		if (which < 0 || (which >= 3 && which != 6 && !(which >= 8 && which < 12) && !b->decode)) return 0;
		if (which < 3) return b->genc->stage_ms(which);
		if (which < 6) return b->gdec->stage_ms(which - 3);
		if (which == 6) return b->genc->stage_ms(0) + b->genc->stage_ms(1) + b->genc->stage_ms(2);
		if (which == 7) return b->gdec->stage_ms(0) + b->gdec->stage_ms(1) + b->gdec->stage_ms(2);
		if (which < 12) return b->genc->entropy().kernel_ms(which - 8);
		if (which < 15) return b->gdec->batch_entropy().kernel_ms(which - 12);
		return 0;
	}
	float ms = 0;                                        // summed over the chunks (each chunk times its own launches with HIP events on its stream)
	for (auto &c : b->chunks) {
		if (which >= 3 && which != 6 && which != 18 && !(which >= 8 && which < 12) && !b->decode) continue;
		if (which < 3) ms += c->enc.last_level_ms(which);
		else if (which < 6) ms += c->dec.last_level_ms(which - 3);
		else if (which >= 8 && which < 12) ms += b->gpu_entropy ? c->enc.entropy().kernel_ms(which - 8) : 0.0f;
		else if (which >= 12 && which < 18) ms += b->gpu_entropy ? c->dec.entropy().kernel_ms(which - 12) : 0.0f;
		else if (which == 18) ms += b->gpu_entropy ? c->enc.entropy().kernel_ms(4) : 0.0f;
		else if (which == 19) ms += b->gpu_entropy ? c->dec.entropy().kernel_ms(6) : 0.0f;
		else ms += which == 6 ? c->enc.last_kernel_ms() : c->dec.last_kernel_ms();
	}
	return ms;
}

// The last completed pass of a stream: rounds, frames coded over all rounds, frames -- a group stream: groups -- whose tables differ from those of the one in front.
int cfhd_amd_batch_stream_stats(cfhd_amd_batch *b, int out[3])
{
	if (!b || !out || !b->stream.on || b->in_flight || !b->stream.stats_valid) return -1;
	for (int k = 0; k < 3; k++) out[k] = b->stream.stats[k];
	return 0;
}

int cfhd_amd_quantizer_is_static(int width, int height, uint32_t pixel_format, int encoded_format, uint32_t encoding_flags, int quality)
{
	FrontEndParams fp;
	if (front_end_params(width, height, pixel_format, encoded_format, encoding_flags, quality, &fp)) return -1;
	return fp.gop ? (fp.gop_static_quantizer ? 1 : 0) : (fp.static_quantizer ? 1 : 0);
}

// which as in cfhd_amd_batch_kernel_ms, 0..5: the name of the transform kernel behind that number (the shape depends on geometry and batch size); 20: k_enc_collect
// (a BYR4 batch: k_enc_collect_bayer, the kernel its planar layouts run)
const char *cfhd_amd_batch_kernel_name(cfhd_amd_batch *b, int which)
{
	if (b && which == 20 && (b->pixel_kind == PIX_YUY2 || b->pixel_kind == PIX_2VUY || b->pixel_kind == PIX_YU64)) return "k_enc_collect_yuv422";      // (the kernel a packed 4:2:2 batch's plane layouts run)
	if (b && which == 20 && (b->pixel_kind == PIX_B64A || b->pixel_kind == PIX_BGRA || b->pixel_kind == PIX_BGRa)) return "k_enc_collect_rgba";      // (... a b64a, BGRA or BGRa batch's)
	if (b && which == 20) return !b->gop && b->pixel_kind == PIX_BYR4 ? "k_enc_collect_bayer" : "k_enc_collect";
	if (b && b->gop) { CallerDevice caller_device; return which < 0 || which > 5 || b->in_flight || (which >= 3 && !b->decode) ? "" : (which < 3 ? b->genc->stage_kernel(which) : b->gdec->stage_kernel(which - 3)); }
	if (!b || which < 0 || which > 5 || b->chunks.empty() || (which >= 3 && !b->decode)) return "";
	return which < 3 ? b->chunks[0]->enc.level_kernel(which) : b->chunks[0]->dec.level_kernel(which - 3);
}

// which: 0 forward (kernels + D2H), 1 host entropy encode + syntax, 2 host parse + entropy decode, 3 H2D + inverse kernels (wall seconds)
double cfhd_amd_batch_stage_seconds(cfhd_amd_batch *b, int which)
{
	if (!b) return 0;
	switch (which) { case 0: return b->t_fwd; case 1: return b->t_entropy_enc; case 2: return b->t_entropy_dec; default: return b->t_inv; }
}

// CFHD_AMD_DX_STATS=1: convergence counters of the chunk-indexed entropy decoder, summed over the chunks (16 words; GpuEntropyDecoder::stats)
int cfhd_amd_batch_dx_stats(cfhd_amd_batch *b, uint32_t *out)
{
	if (!b || b->in_flight || !out || b->gop) return -1;      // (group batches have no chunk-indexed decoder)
	for (int k = 0; k < 16; k++) out[k] = 0;
	int rc = -1;
	if (b->decode) for (auto &c : b->chunks) { uint32_t s[16]; if (c->dec.entropy().stats(s) == 0) { rc = 0; for (int k = 0; k < 16; k++) out[k] = k == 2 ? (s[k] > out[k] ? s[k] : out[k]) : out[k] + s[k]; } }
	return rc;
}

int cfhd_amd_batch_get_sample(cfhd_amd_batch *b, int i, const void **data, size_t *size)
{
	if (!b || b->in_flight || i < 0 || i >= b->n || !data || !size) return -1;
	if (b->gop) {                                       // sample 2 g: group g; 2 g + 1: the P-frame sample behind it
		*data = (i & 1) ? (const void *)(b->pframes.data() + (size_t)kPFrameSampleBytes * (i / 2)) : (const void *)b->genc->entropy().host_sample(i / 2);
		*size = b->sample_size[i];
		return 0;
	}
	int l; cfhd_amd_chunk &c = b->chunk_of(i, &l);
	*data = b->gpu_entropy ? (const void *)c.enc.entropy().host_sample(l) : (const void *)b->samples[i].data(); *size = b->sample_size[i];
	return 0;
}

int cfhd_amd_batch_download_output(cfhd_amd_batch *b, int i, void *out, int pitch)
{
	CallerDevice caller_device;
	if (!b || b->in_flight || i < 0 || i >= b->n || !b->decode) return -1;
	if (b->gop) { if (b->gdec->download_frame(i, out, pitch) || b->gdec->wait()) return -2; return b->gdec->finish_frame(i, out, pitch); }
	int l; cfhd_amd_chunk &c = b->chunk_of(i, &l);
	if (c.dec.download_frame(l, out, pitch) || c.dec.wait()) return -2;
	return c.dec.finish_frame(l, out, pitch);
}

// The 40-byte sequence header a stream of two-frame groups starts with (what a CFHD_EncodeSample handle answers its first call with); -1 for a batch without groups.
// The batch's samples, pass after pass, are that handle's stream with this header taken out.
int cfhd_amd_batch_get_sequence_header(cfhd_amd_batch *b, const void **data, size_t *size)
{
	if (!b || b->in_flight || !b->gop || !data || !size) return -1;
	*data = b->sequence_header; *size = b->sequence_header_size;
	return 0;
}

} // extern "C"
