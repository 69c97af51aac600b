// cfhd_device.h -- GPU side of the codec: batches of frames in flight (HIP stream + HBM buffers + job tables)
// and the launch sequences for encode (forward transform) and decode (inverse transform).
#pragma once
#include "cfhd_core.h"
#include "cfhd_bitstream.h"
#include "cfhd_entropy_gpu.h"
#include "cfhd_gop.h"
#include <stdint.h>
#include <stddef.h>
#include <vector>

namespace cfhd {

// 0 on success; otherwise a hipError_t value.  The product has no CPU fallback: callers turn a failure into
// CFHD_ERROR_INTERNAL and the message is available from device_last_error().
int device_init();                 // picks the device from CFHD_AMD_DEVICE, else LOCAL_RANK, else 0
int device_count();
int device_select(int dev);        // this thread prepares its batches on device `dev` from now on (-1: the process default again); returns the device in effect, -1 on failure
int device_current();              // the device device_init() puts this thread on
// Passes that are queued as a whole (cfhd_amd_batch_submit) can take turns per stage on a device: the encode half of a pass starts behind the encode half of the pass queued
// before it on that device (the default for encode-only passes: cfhd_batch.cpp batch_launch says why) and, with CFHD_AMD_QUEUE=ordered, the decode half behind that pass's
// decode half.  stage 0: encode, 1: decode.  stage_order_wait: work queued on
// `stream` from now on waits for the last stage_order_done of that stage on `device`; stage_order_done: the work `stream` holds now is that stage's latest.
int stage_order_wait(int device, int stage, void *stream);
int stage_order_done(int device, int stage, void *stream);
// Passes in flight on a device: a queue raises the count when it queues a pass (cfhd_amd_batch_submit and its variants, the decode queue's submits) and lowers it
// when the pass is collected or fails; the synchronous entry points never touch it.  Read on the host when a pass is queued, by launches that claim less of the chip
// while other passes wait for room beside them (GpuEntropyDecoder::launch_dx).  A hint, never a correctness input: nothing orders a reader against a writer.
void device_pass_begin(int device);
void device_pass_end(int device);
int device_passes_in_flight(int device);
// The HIP device the calling thread had current when it entered the library, put back when it leaves: a handle that was dealt another GPU (unit_device)
// must not leave the application's thread on that GPU -- its own HIP / PyTorch work would land there.  Every public entry point that can select a device holds one.
int device_caller_save();          // the caller's current device, -1 when there is none to restore
void device_caller_restore(int dev);
struct CallerDevice { int dev; CallerDevice() : dev(device_caller_save()) {} ~CallerDevice() { device_caller_restore(dev); } CallerDevice(const CallerDevice &) = delete; };
const char *device_last_error();
void device_set_last_error(const char *text);      // a refusal decided on the host that the caller should be able to read (cfhd_amd_last_error)

// The HIP-event times of the k_enc_collect launches (cfhd_collect_kernels.h: frames from planar tensors in device memory) that feed a frame-queue pass, for EncodeBatch
// and GopBatch alike.  A call of upload_frames_device_planar records a pair of events around its launch; begin_pass() (the pass's first launch) closes the set that
// fed it, the first wait() behind it sums the set into `ms` -- 0 for a pass no such call fed.  A batch that is never fed this way makes and records no event.
struct CollectTimes {
	std::vector<void *> ev;             // pairs, made when first needed
	int recorded = 0, in_pass = 0; bool open = false; float ms = 0;
	int record(void *stream, bool end);      // the event in front of (end = false) / behind (true: the pair is complete) a launch on `stream`; 0 or a hipError_t
	void begin_pass() { if (!open) { open = true; in_pass = recorded; recorded = 0; } }
	void resolve();                     // behind a stream synchronise
	void release();
};

// N frames that travel through the forward path together: one launch per wavelet level covers every channel of
// every frame (blockIdx.z walks the job table).  N = 1 is the synchronous CFHD_EncodeSample path.
struct ForwardRoute; struct InverseRoute; struct GopRoute; enum class FwdL1;      // (cfhd_device.hip: the kernels a launch picks)
class EncodeBatch {
public:
	EncodeBatch();
	~EncodeBatch();
	int prepare(const FramePlan &plan, int nframes);      // allocates HBM and pinned host staging for the packed frames, the pyramids and the job tables
	int nframes() const { return n_; }
	const FramePlan &plan() const { return plan_; }
	// Stage one host frame (any pitch, negative allowed as in Codec/encoder.c:1957) and start its H2D copy.
	int upload_frame(int i, const void *frame, int pitch_bytes);
	int upload_frame_device(int i, const void *d_frame, int pitch_bytes);      // the same for a frame in HBM on the batch's device: one strided D2D copy on the batch's stream, no staging
	int upload_frames(const void *frames, size_t frame_stride, int pitch_bytes);      // all n frames, asynchronous on the batch's stream; ONE copy when the frames lie back to back in a registered buffer
	// frames first .. first + count - 1 of an RG48 batch from planar R, G, B tensors in HBM on the batch's device (layout: dev::COLLECT_PLANAR_*; frame first + k at
	// d_frames + k * frame_stride, rows row_pitch apart, planes display_height * row_pitch apart): ONE k_enc_collect launch on the batch's stream, no staging, no host
	// wait.  -1 with the reason in device_last_error() for what the gates refuse (cfhd_amd_batch_upload_device_planar lists them); a hipError_t for a device failure.
	int upload_frames_device_planar(int first, int count, const void *d_frames, size_t frame_stride, int row_pitch, int layout);
	void collect_begin_pass() { collect_.begin_pass(); }      // the frame queue calls this in front of a pass's first launch
	float collect_ms() const { return collect_.ms; }          // k_enc_collect launches that fed the last completed pass (0: none did)
	int download_input_frame(int i, void *out, int pitch_bytes);      // frame i as the batch holds it, packed: a strided D2H copy behind what the stream holds, waited for
	// the next launches (forward transform, entropy coder, sample download) cover frames 0 .. k-1 only (0 = all)
	void set_active(int k) { active_ = k; ent_.set_active(k); }
	// async: all levels, all frames.  coeffs_needed = false: nothing but the GPU entropy stage will read this launch's coefficients -- where the level-1 bands
	// leave as block lists (k_fwd_yuv422_strip_blocks, cfhd_kernels.h FwdBlockLists) their dense rows are then not written at all.
	int launch_forward(bool coeffs_needed = true) { return launch_forward(coeffs_needed, 0, 0); }
	// the same over a window of the batch, frames first .. first + count - 1 (count 0: frames 0 .. active - 1): the job tables from `first` on, grids sized by count, the
	// kernels a batch of count frames would pick.  The block lists and the pyramids are the frames' own, numbered over the whole batch.
	int launch_forward(bool coeffs_needed, int first, int count);
	int update_quant(const FramePlan &plan);           // same geometry, new quantizer tables for every frame (per-frame rate feedback of the handles)
	// new quantizer tables for frame i alone (the frame queue's rate-feedback streams: every frame of a pass carries its own).  The caller has drained the stream.
	int set_frame_quant(int i, const FramePlan &plan);
	const FramePlan &frame_plan(int i) const { return frame_plans_.empty() ? plan_ : frame_plans_[i]; }
	// GPU entropy stage (cfhd_entropy_kernels.h): complete samples are produced in HBM after launch_forward().
	int prepare_entropy(size_t sample_cap);
	GpuEntropyEncoder &entropy() { return ent_; }
	void set_stage_pieces(int k) { stage_pieces_ = k < 1 ? 1 : (k > 16 ? 16 : k); }      // plain input frames staged in k pieces (upload_frame)
	bool has_entropy() const { return ent_ready_; }
	// name of the kernel the next launch_forward(coeffs_needed) uses for level 0 / 1 / 2 (as a profiler shows it; two launches: "a+b")
	const char *level_kernel(int level, bool coeffs_needed = false) const;
	int download_coeffs();                             // async: final (entropy coded) region of every frame -> pinned host
	int wait();
	const int16_t *host_coeffs(int i) const { return h_coeff_ + (size_t)i * plan_.final_elems; }
	int16_t *device_coeffs(int i) { return d_coeff_ + (size_t)i * plan_.coeff_elems; }
	void *stream() { return stream_; }
	int device() const { return device_; }
	float last_kernel_ms() const { return kernel_ms_; }   // forward kernels of the last launch (HIP events on this stream)
	float last_level_ms(int level) const { return level_ms_[level]; }   // level 0 = k_fwd_yuv422, 1/2 = k_fwd_plane launches
	void release();                                    // frees every device / pinned buffer of the batch (the destructor's work; prepare() starts with it)
private:
	int sync_jobs();
	void fill_jobs();
	void fill_frame_jobs(int i);                    // frame i's rows of the job tables, from frame_plan(i)
	void fill_block_lists();
	ForwardRoute forward_route(bool coeffs_needed, int frames) const;      // which kernels a launch_forward() over `frames` frames runs: launch_forward() and level_kernel() both read this
	FramePlan plan_;
	std::vector<FramePlan> frame_plans_;            // empty: every frame carries plan_'s divisors; else frame i its own (set_frame_quant)
	int n_ = 0, active_ = 0, device_ = 0; bool jobs_dirty_ = true;
	void *stream_ = nullptr, *ev0_ = nullptr, *ev1_ = nullptr, *evl_[2] = {nullptr, nullptr};
	float level_ms_[3] = {0, 0, 0};
	uint8_t *d_in_ = nullptr, *h_in_ = nullptr; size_t frame_bytes_ = 0; int in_pitch_ = 0, in_rows_ = 0;
	int16_t *d_coeff_ = nullptr, *h_coeff_ = nullptr;
	void *d_jobs_ = nullptr, *h_jobs_ = nullptr; size_t jobs_bytes_ = 0;
	int16_t *d_planes_ = nullptr; uint16_t *d_curve_ = nullptr; size_t plane_elems_ = 0;   // Bayer input: component planes + encode curve LUT
	// Bayer: k_unpack_byr4 writes the component planes and k_fwd_plane transforms them (small launches; large ones take k_fwd_bayer_strip, level 1 straight from the mosaic)
	float kernel_ms_ = 0;
	bool timed_ = false;
	GpuEntropyEncoder ent_; bool ent_ready_ = false;
	int stage_pieces_ = 1;
	CollectTimes collect_;
};

// What a decoder output needs, computed once from (the sample's encoded format, the requested output, half, interlaced) by output_route() in cfhd_device.hip -- the one
// place that knows what an output means.  DecodeBatch keeps it from prepare() on and sizes its buffers, builds its one last-level job table, names its kernel and runs
// its conversion from it; GopBatch asks the same function for the outputs of 4:2:2 samples.  A new output format is a new answer of output_route(), at most one job
// helper and at most one case of launch_convert().  (Which widths a caller may ask for is the C ABI's gate: cfhd_api_decoder.inc yuv422_output_served.)
enum class OutJobs { Yuv, Planes16, HalfYuv, HalfPacked };      // the table the last launch reads: InvYuvJob | InvPlaneJob per output plane | HalfYuvJob | HalfPackedJob
enum class OutConvert { None, V210, Rgb24, Rgb16, Byr4 };       // the pass behind the last level (k_yu64_to_v210 / _rgb24 / _rgb16, k_bayer_to_byr4); any but None: the last level writes a scratch frame (Byr4: unless k_inv_bayer_strip runs)
struct OutputRoute {
	const char *refusal = nullptr;                  // not served: the text device_last_error() gives, prepare() answers -2
	int width_multiple = 1; const char *width_refusal = nullptr;      // the output's width in pixels is a multiple of this, or the same answer with this text
	OutJobs jobs = OutJobs::Yuv;
	int work = 0;                                   // the pixel kind the last-level kernel writes: the output itself, YU64 rows in front of a conversion, RG48 words of four planes for BYR4
	OutConvert convert = OutConvert::None; int rgb16_mode = 0;       // k_yu64_to_rgb16: 0 RG48, 1 b64a, 2 BGRa, 3 BGRA
	// half resolution: HalfYuvJob::mode and bottom_up (k_half_rgb24); HalfPackedJob::mode (0: k_half_packed16, else k_half_rgb), bytes, bottom_up and big_endian
	int half_mode = 0, half_bytes = 0; bool bottom_up = false, big_endian = false;
	int lowpass_kind = 0;                           // the output as the lowpass bias rule sees it (lowpass_bias()): the requested kind
};

class DecodeBatch {
public:
	DecodeBatch();
	~DecodeBatch();
	// half: CFHD_DECODED_RESOLUTION_HALF of 4:2:2 samples -- the last wavelet level is not run, the level-1 lowpass planes are the picture
	int prepare(const FramePlan &plan, int nframes, int out_pixel_kind, bool half = false);
	// interlaced 4:2:2 samples: the last level is the inverse frame transform (k_inv_frame_yuv422; 8-bit 4:2:2 output, full resolution), or into 16-bit rows
	// (k_inv_frame_yuv422_rows16) for RG48 / b64a / BGRA / BGRa; set before prepare()
	void set_interlaced(bool on) { interlaced_ = on; ent_.set_interlaced(on); }
	bool interlaced() const { return interlaced_; }
	// BYR4 output: large launches write the mosaic straight from the last level (k_inv_bayer_strip) where the geometry fits; off, the default, keeps the pair
	// k_inv_packed16 + k_bayer_to_byr4 at every size (the C ABI's handles).  Set by the queues' Bayer batches (cfhd_amd_decode_batch_create_bayer, cfhd_amd_batch_create_bayer).
	void set_bayer_strips(bool on) { bayer_strips_ = on; }
	// the next launches (entropy decoder with host-parsed samples, inverse transform) cover frames 0 .. k-1 only (0 = all)
	void set_active(int k) { active_ = k; ent_.set_active(k); }
	int nframes() const { return n_; }
	const FramePlan &plan() const { return plan_; }
	int16_t *host_coeffs(int i) { return h_coeff_ + (size_t)i * plan_.final_elems; }   // host entropy decoder writes here
	int16_t *device_coeffs(int i) { return d_coeff_ + (size_t)i * plan_.coeff_elems; }
	void clear_host_coeffs(int i);
	int upload_coeffs();                               // async: pinned host -> HBM (final region of every frame)
	// GPU entropy decoder (k_dec_bands): samples in, dequantized pyramid built in HBM (replaces host_coeffs()/upload_coeffs()).
	int prepare_entropy(size_t sample_cap);
	GpuEntropyDecoder &entropy() { return ent_; }
	int launch_entropy();                            // entropy().launch() with the level-1 bands as block lists where the inverse gathers them
	bool has_entropy() const { return ent_ready_; }
	const char *level_kernel(int level) const;      // name of the kernel the next launch_entropy() + launch_inverse() use for level 0 / 1 / 2 (as a profiler shows it)
	int launch_inverse(uint32_t dither_seed);          // async
	int download_frame(int i, void *out, int pitch_bytes);   // async D2H into pinned staging, then row copy after wait
	int download_frames(void *out, size_t frame_stride, int pitch_bytes);      // all n frames -- the first k after set_active(k) -- (finish_frame() for each behind wait()); ONE copy into a registered buffer that takes them back to back
	// the decoded pictures in HBM, for a kernel queued behind launch_inverse() on stream() (the decode queue's k_dec_blank): picture i at device_pictures() + i * picture_bytes()
	uint8_t *device_pictures() const { return d_out_; }
	size_t picture_bytes() const { return frame_bytes_; }
	int picture_pitch() const { return out_pitch_; }
	int picture_rows() const { return out_rows_; }
	int after(void *producer_stream);                  // async: later work on this batch's stream waits for what the producer stream holds now
	int wait();
	int finish_frame(int i, void *out, int pitch_bytes);      // after wait(): copy the staged frame to the caller's buffer
	void *stream() { return stream_; }
	float last_kernel_ms() const { return kernel_ms_; }
	float last_level_ms(int level) const { return level_ms_[level]; }   // level 0 = k_inv_yuv422, 1/2 = k_inv_plane launches (level index)
	void release();                                    // frees every device / pinned buffer of the batch (the destructor's work; prepare() starts with it)
private:
	int sync_jobs();
	InverseRoute inverse_route() const;             // which kernels the next launch_entropy() + launch_inverse() run: both and level_kernel() read this
	FramePlan plan_;
	int n_ = 0, device_ = 0; bool jobs_dirty_ = true, half_ = false, interlaced_ = false, bayer_strips_ = false; int active_ = 0;
	int out_kind_ = 0; OutputRoute route_;          // the REQUESTED output kind, never rewritten, and what it needs (the kind the kernels write is route_.work)
	void *stream_ = nullptr, *ev0_ = nullptr, *ev1_ = nullptr, *evl_[2] = {nullptr, nullptr};
	float level_ms_[3] = {0, 0, 0};
	int16_t *d_coeff_ = nullptr, *h_coeff_ = nullptr;
	uint8_t *d_out_ = nullptr, *h_out_ = nullptr; size_t frame_bytes_ = 0; int out_pitch_ = 0, out_rows_ = 0;
	uint8_t *d_tmp_ = nullptr; int tmp_pitch_ = 0; size_t tmp_frame_bytes_ = 0;      // outputs behind a conversion (route_.convert): the scratch frames the last level writes
	// levels 3 and 2 of the inverse transform on a stream of their own when the entropy decoder finished their bands ahead of the level-1 bands (GpuEntropyDecoder::levels23_event)
	void *stream2_ = nullptr, *ev2_[3] = {nullptr, nullptr, nullptr}; bool inv_split_ = false;
	uint16_t *d_restore_ = nullptr;                 // BYR4 output: the linear-restore table of k_bayer_to_byr4 in HBM
	std::vector<char> direct_;                      // frame i went straight to the caller's (registered) buffer: finish_frame has nothing to copy
	enum { kMaxOutPieces = 8 };
	int stage_pieces_ = 1;
public:
	// plain host buffers staged in k pieces (download_frame / finish_frame: the CPU copy of a piece beside the DMA of the next); then finish_frame() may be called before wait()
	void set_stage_pieces(int k) { stage_pieces_ = k < 1 ? 1 : (k > kMaxOutPieces ? (int)kMaxOutPieces : k); }
	bool staged_in_pieces() const { return stage_pieces_ > 1; }
private:
	std::vector<void *> piece_ev_; std::vector<int> out_pieces_;     // frames staged in pieces (download_frame / finish_frame): an event behind every piece's DMA
	void *d_jobs_ = nullptr, *h_jobs_ = nullptr; size_t jobs_bytes_ = 0;
	float kernel_ms_ = 0;
	bool timed_ = false;
	void *evdep_ = nullptr;
	GpuEntropyDecoder ent_; bool ent_ready_ = false;
};

// n two-frame groups on the GPU (cfhd_gop.h; n = 1: the C ABI's handles, n > 1: the group batches of cfhd_batch.cpp): the kernels of the intra path (level 1 of all
// 2 n frames -- from every input that encodes to 4:2:2 --, the plane transforms of the three spatial wavelets) around the temporal step, forward for the encoder and
// inverse for the decoder, one launch per stage whatever n is (the job tables are n times as long, the job index stays in blockIdx.y / z).  The run-length / VLC stage
// runs on the device too: GpuEntropyEncoder::prepare_group codes the n group samples, the decoder of a batch parses and decodes them where the coder left them
// (GpuGroupBatchEntropyDecoder), the decode queue brings group samples of any encoder in slots of their own (cfhd_decode_queue.hip), the C ABI's decoder takes one host-parsed sample (GpuGroupEntropyDecoder); the host writer / host VLC decoder remain for what the device
// stage hands back (write_group_sample / vlc_decode_band: the pyramid crosses PCIe then).
class GopBatch {
public:
	GopBatch();
	~GopBatch();
	// decode: out_pixel_kind is any output a 4:2:2 sample decodes to (OutputRoute: the last level of both frames is the intra path's job and kernel of that output); half: the
	// level-1 lowpass planes the temporal inverse leaves are the picture (CFHD_DECODED_RESOLUTION_HALF), the last level is not run
	// ngroups: frames 2 g and 2 g + 1 form group g; pyramids plan.coeff_elems apart.  A count whose job index would pass the grid limit (65 535) is refused.
	int prepare(const GopPlan &plan, bool decode, int out_pixel_kind, bool half = false, int ngroups = 1);
	const GopPlan &plan() const { return plan_; }
	int ngroups() const { return n_; }
	void set_color_matrix(int m);                    // decoder: the matrix of the outputs that convert to RGB (FramePlan::color_matrix), from the group sample's colour space tag
	void set_plan(const GopPlan &plan);              // same geometry, new quantizer tables
	// Group g's divisors alone (the frame queue's group streams: every group carries tables of its own, EncodeBatch::set_frame_quant's twin): its rows of the job tables
	// are rewritten and travel to the device with the next launch, the rows of the other groups neither.  The sample header is the caller's
	// (GpuEntropyEncoder::set_group_plan + set_frame_header); the pinned job table must not be in flight.
	int set_group_plan(int g, const GopPlan &plan);
	const GopPlan &group_plan(int g) const { return group_plans_.empty() ? plan_ : group_plans_[(size_t)g]; }
	// encoder
	int upload_frame(int f, const void *frame, int pitch_bytes);      // f = 0 .. 2 n - 1: stage one frame and start its H2D copy
	int upload_frame_device(int f, const void *d_frame, int pitch_bytes);      // the same for a frame in HBM on the batch's device: one strided D2D copy on the batch's stream
	int upload_frames(const void *frames, size_t frame_stride, int pitch_bytes);      // all 2 n frames, asynchronous on the batch's stream (staged through pinned memory unless registered and back to back)
	// EncodeBatch::upload_frames_device_planar / collect_begin_pass / collect_ms / download_input_frame for the 2 n frames of the groups
	int upload_frames_device_planar(int first, int count, const void *d_frames, size_t frame_stride, int row_pitch, int layout);
	void collect_begin_pass() { collect_.begin_pass(); }
	float collect_ms() const { return collect_.ms; }
	int download_input_frame(int f, void *out, int pitch_bytes);
	int launch_forward() { return launch_forward(0, n_); }      // async: level 1 of all frames, temporal step, three spatial transforms per channel
	// the same over groups first_group .. first_group + count - 1: the job tables are group-major, so a window is every table from its first group's rows on and grids
	// sized by count; (0, n) is launch_forward()
	int launch_forward(int first_group, int count);
	const char *level1_kernel() const;               // name of the kernel the next launch_forward() runs for level 1 of both frames (as a profiler shows it)
	int download_coeffs();                           // async: the group pyramid -> pinned host
	// GPU entropy stage for the group sample (GpuEntropyEncoder::prepare_group): entropy().set_frame_header(0, hdr), launch_forward(), entropy().launch(),
	// entropy().download(), wait() -> entropy().host_sample(0)
	int prepare_entropy(size_t sample_cap);
	bool has_entropy() const { return ent_ready_; }
	GpuEntropyEncoder &entropy() { return ent_; }
	const int16_t *host_coeffs() const { return h_coeff_; }
	// decoder
	int16_t *host_coeffs_rw() { return h_coeff_; }   // the host entropy decoder writes the dequantized bands here
	// GPU entropy decode of a parsed group sample into the pyramid in HBM (GpuGroupEntropyDecoder); < 0: not served / malformed, decode on the host instead
	int launch_entropy_decode(const uint8_t *sample, size_t size, const ParsedGroup &pg, size_t sample_cap);
	int entropy_decode_errors() { return dec_.check(); }                    // after wait()
	// a batch of groups whose samples lie in HBM (the coder's dense buffer): parsed and decoded there, nothing touches the host; then launch_inverse(seed, true)
	int prepare_entropy_decode();
	GpuGroupBatchEntropyDecoder &batch_entropy() { return bdec_; }
	// the next launches of the decoder (batch_entropy().launch(), launch_inverse(), download_frames()) cover groups 0 .. k-1 only (0 = all): pictures 0 .. 2 k - 1
	void set_active(int k) { active_ = k; bdec_.set_active(k); }
	// the decoded pictures in HBM, for a kernel queued behind launch_inverse() on stream() (the decode queue's k_dec_blank): picture f at device_pictures() + f * picture_bytes()
	uint8_t *device_pictures() const { return d_frames_; }
	size_t picture_bytes() const { return frame_bytes_; }
	int picture_pitch() const { return pitch_; }
	int picture_rows() const { return rows_; }
	int16_t *device_coeffs() { return d_coeff_; }
	void *stream() { return stream_; }
	int device() const { return device_; }
	int download_frames(void *out, size_t frame_stride, int pitch_bytes);      // all 2 n frames -- the first 2 k after set_active(k) -- (finish_frame() for each behind wait())
	// HIP-event times of the last launch_forward() / launch_inverse() once the stream was synchronised, and the kernels behind them.  Forward: 0 level 1 of all frames,
	// 1 temporal step + the two middle wavelets, 2 the top wavelet.  Inverse: 0 last level of all frames (+ output conversion), 1 the two middle wavelets + temporal
	// step, 2 the top wavelet.  set_timed(true) before the launches (the C ABI's handles record no events).
	void set_timed(bool on);
	float stage_ms(int k);
	const char *stage_kernel(int k) const;
	int launch_inverse(uint32_t dither_seed, bool coeffs_on_device = false);      // async: (pyramid H2D,) three inverse spatial transforms, temporal step, last level of both frames
	int download_frame(int f, void *out, int pitch_bytes);
	int finish_frame(int f, void *out, int pitch_bytes);
	int wait();
	void release();
private:
	void fill_jobs();
	void fill_group_jobs(int g);                     // group g's rows of the job tables, from group_plan(g)
	int sync_jobs();                                 // the whole table, or the rows of the groups set_group_plan() rewrote
	std::vector<GopPlan> group_plans_;               // empty: every group carries plan_'s divisors; else group g its own (set_group_plan)
	std::vector<char> group_dirty_;                  // encoder: groups whose rows differ from the device's copy
	GopRoute route() const;                          // decoder: output_route() of a 4:2:2 sample for the output kind, half and interlaced, and the kernel that serves its family
	FwdL1 forward_route() const;                     // encoder: the level-1 kernel of both frames, from the input kind and interlaced alone
	GopPlan plan_; bool decode_ = false, half_ = false; int out_kind_ = 0, device_ = 0, matrix_ = 0, n_ = 1, active_ = 0;
	int active_groups() const { return active_ > 0 && active_ < n_ ? active_ : n_; }
	void *stream_ = nullptr, *ev_[4] = {nullptr, nullptr, nullptr, nullptr}; bool timed_ = false, launched_ = false; mutable char stage_name_[3][64];
	uint8_t *d_frames_ = nullptr, *h_frames_ = nullptr; size_t frame_bytes_ = 0; int pitch_ = 0, rows_ = 0;
	// decoder outputs behind a conversion (OutputRoute::convert): the YU64 rows of both frames first
	uint8_t *d_tmp_ = nullptr; size_t tmp_frame_bytes_ = 0; int tmp_pitch_ = 0;
	int16_t *d_coeff_ = nullptr, *h_coeff_ = nullptr;
	void *d_jobs_ = nullptr, *h_jobs_ = nullptr; size_t jobs_bytes_ = 0; bool jobs_dirty_ = true;
	GpuEntropyEncoder ent_; bool ent_ready_ = false;
	GpuGroupEntropyDecoder dec_; bool dec_ready_ = false;
	GpuGroupBatchEntropyDecoder bdec_; bool bdec_ready_ = false;
	CollectTimes collect_;
};

int packed_frame_pitch(int pixel_kind, int width);     // bytes per row of a tightly packed frame

// Host buffers the caller promised to keep alive (cfhd_amd_register_host_buffer): page-locked once, then frames and samples travel between
// them and HBM without the staging copy through the library's own pinned memory.  Everything else is staged.
int host_buffer_register(void *p, size_t bytes);       // 0, or a hipError_t
int host_buffer_unregister(void *p);
bool host_buffer_is_registered(const void *p, size_t bytes);


} // namespace cfhd
