// cfhd_entropy_gpu.hip -- see cfhd_entropy_gpu.h
#include "cfhd_entropy_gpu.h"
#include "cfhd_entropy_jobs.h"
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

namespace cfhd {

int device_init();
int device_current();
int device_passes_in_flight(int device);      // (cfhd_device.h)
namespace { int g_fail(hipError_t e, const char *what) { fprintf(stderr, "[cfhd_amd] %s: %s\n", what, hipGetErrorString(e)); return (int)e ? (int)e : -1; } }
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return g_fail(_e, #expr); } while (0)
// workgroups per CU of k_dec_index / k_dec_tiles beside other passes in flight (GpuEntropyDecoder::prepare; alone: 5 and 3, all that fit)
enum { kDxSharedIndexPerCu = 2, kDxSharedTilesPerCu = 2 };

struct GpuEntropyEncoder::Host { EntHostJobs jobs; std::vector<EntHoleGeom> geom; dev::EntFrameJob *frames = nullptr; /* pinned: async copies must not stall the host */ };

GpuEntropyEncoder::GpuEntropyEncoder() : host_(new Host) {}
GpuEntropyEncoder::~GpuEntropyEncoder() { release(); delete host_; }

void GpuEntropyEncoder::release()
{
	(void)hipSetDevice(device_);
	void *dev[] = { d_sizes_, d_tables_, d_bands_, d_segband_, d_segs_, d_bandstate_, d_frames_, d_tmpl_, d_packed_, d_offsets_, d_tokens_, d_blocks_, d_masks_, d_scratch_ };
	for (void *p : dev) if (p) (void)hipFree(p);
	d_scratch_ = nullptr; scratch_stride_ = 0;
	if (h_samples_) (void)hipHostFree(h_samples_);
	if (h_sizes_) (void)hipHostFree(h_sizes_);
	if (h_offsets_) (void)hipHostFree(h_offsets_);
	d_packed_ = nullptr; d_offsets_ = h_offsets_ = nullptr;
	if (h_tmpl_) (void)hipHostFree(h_tmpl_);
	if (host_->frames) { (void)hipHostFree(host_->frames); host_->frames = nullptr; }
	for (void *&e : ev_) if (e) { (void)hipEventDestroy((hipEvent_t)e); e = nullptr; }
	for (void *&e : ev2_) if (e) { (void)hipEventDestroy((hipEvent_t)e); e = nullptr; }
	if (stream2_) { device_stream_destroy(stream2_); stream2_ = nullptr; }
	timed_ = false;
	h_samples_ = nullptr; d_sizes_ = h_sizes_ = nullptr; d_tables_ = d_bands_ = d_segband_ = d_segs_ = d_bandstate_ = d_frames_ = d_tokens_ = nullptr;
	d_tmpl_ = h_tmpl_ = nullptr; n_ = 0;
	d_blocks_ = nullptr; d_masks_ = nullptr; masks_per_frame_ = 0; use_blocks_ = false;
}

int GpuEntropyEncoder::prepare(const FramePlan &plan, int nframes, int16_t *d_coeffs, size_t stride, size_t sample_cap, void *stream)
{
	group_ = false; plan_ = plan;
	return prepare_units(nframes, d_coeffs, stride, sample_cap, stream);
}

// Two-frame groups (cfhd_gop.h): one group per unit, 17 subbands per channel -- the same kernels over the group's template and band table.
int GpuEntropyEncoder::prepare_group(const GopPlan &plan, int ngroups, int16_t *d_coeffs, size_t stride, size_t sample_cap, void *stream)
{
	group_ = true; gplan_ = plan; plan_ = FramePlan(); plan_.interlaced = false;
	return prepare_units(ngroups, d_coeffs, stride, sample_cap, stream);
}

void GpuEntropyEncoder::build_template(const SampleHeaderInfo &hdr, SampleTemplate *t) const
{
	if (group_) build_group_template(gplan_, hdr, t); else build_sample_template(plan_, hdr, t);
}

int GpuEntropyEncoder::prepare_units(int nframes, int16_t *d_coeffs, size_t stride, size_t sample_cap, void *stream)
{
	int rc = device_init();
	if (rc) return rc;
	release();
	device_ = device_current(); (void)hipSetDevice(device_);
	const FramePlan &plan = plan_;
	n_ = nframes; cap_ = (sample_cap + 255) & ~(size_t)255; stream_ = stream; d_coeffs_ = d_coeffs; coeff_stride_ = stride;
	if (cap_ * (size_t)n_ >= ((size_t)1 << 32)) { fprintf(stderr, "[cfhd_amd] batch of %d frames exceeds the 4 GiB sample arena\n", n_); return -5; }   // packed offsets are 32-bit
	{
		std::vector<dev::EntTables> h(2);
		ent_build_tables(&h[0], 1); ent_build_tables(&h[1], 2);
		HIPCHK(hipMalloc(&d_tables_, 2 * sizeof(dev::EntTables)));
		HIPCHK(hipMemcpy(d_tables_, h.data(), 2 * sizeof(dev::EntTables), hipMemcpyHostToDevice));
	}
	SampleHeaderInfo hdr0 = { 1, 2, 2, 4, !plan.interlaced, nullptr, 0, nullptr, 0 };
	tmpl_.assign(n_, SampleTemplate());
	build_template(hdr0, &tmpl_[0]);
	EntHostJobs &jobs = host_->jobs;
	host_->geom = group_ ? ent_hole_geometry(gplan_, tmpl_[0]) : ent_hole_geometry(plan, tmpl_[0]);
	// block lists of the level-1 bands, for the geometries k_fwd_yuv422_strip_blocks serves (EncodeBatch::forward_route): one 16-byte slot per block of the
	// pyramid (only the slots of listed blocks are ever touched), one mask per chunk
	const bool lists = !group_ && !plan.interlaced && plan.encoded_format == ENC_YUV422 && (plan.pixel_kind == PIX_YUY2 || plan.pixel_kind == PIX_2VUY) && plan.width % 32 == 0;
	// Those bands are sparse (a level-1 segment of 1024 coefficients codes ~400 bits): segments of dev::ENT_SEG_L1 coefficients there, so that the fixed cost of a wave in
	// k_ent_count_blocks / k_ent_emit is paid a quarter as often.  CFHD_AMD_L1_SEG=1024 .. 8192 (multiples of 1024): another length, for A/B runs and the sweep.
	static const int l1_seg_env = [] { const char *e = getenv("CFHD_AMD_L1_SEG"); const int v = e ? atoi(e) : 0;
	                                   return v >= dev::ENT_SEG && v <= dev::ENT_SEG_MAX && v % dev::ENT_SEG == 0 ? v : (int)dev::ENT_SEG_L1; }();
	// The bands k_ent_count counts densely pay the same fixed cost per wave: cfhd_entropy_jobs.h EntSegRule, one length per level.  Long segments trade waves for fixed
	// cost, which pays once the launches have more waves than the chip holds at a time (256 CUs x 4 SIMDs x 8 waves of k_ent_count / k_ent_emit); a pass below that -- a
	// single frame of the C ABI, a few small ones -- runs all its waves side by side and takes as long as its longest wave: it keeps dev::ENT_SEG.
	// CFHD_AMD_SEG_L1_DENSE, CFHD_AMD_SEG_L2, CFHD_AMD_SEG_L3 = 1024 .. 8192 (multiples of 1024): that length whatever the size of the pass; read at every prepare, so that
	// one process can hold encoders of different lengths (tests, sweeps).
	enum { kWaveSlots = 256 * 4 * 8 };
	const bool fills_chip = (size_t)n_ * stride / dev::ENT_SEG >= (size_t)kWaveSlots;
	auto seg_env = [&](const char *name, int dflt) { const char *e = getenv(name); const int v = e ? atoi(e) : 0; return ent_seg_len_ok(v) ? v : (fills_chip ? dflt : (int)dev::ENT_SEG); };
	const EntSegRule rule = { seg_env("CFHD_AMD_SEG_L1_DENSE", dev::ENT_SEG_L1_DENSE), seg_env("CFHD_AMD_SEG_L2", dev::ENT_SEG_L2), seg_env("CFHD_AMD_SEG_L3", dev::ENT_SEG_L3), lists };
	// a group whose subband 7 is coded in two passes (8-bit RGB sources): the planes k_ent_split_two_pass fills for the two holes of every channel, the encoder's own
	scratch_stride_ = group_ ? ent_scratch_stride(gplan_) : 0;
	if (scratch_stride_) {
		dev::EntSplitJob probe;
		if (!ent_split_job(gplan_, d_coeffs, stride, nullptr, &probe)) return -3;
		HIPCHK(hipMalloc((void **)&d_scratch_, scratch_stride_ * 2 * (size_t)n_));
	}
	if (!ent_build_band_jobs(host_->geom, tmpl_[0], n_, d_coeffs, stride, &jobs, lists ? l1_seg_env : (int)dev::ENT_SEG, &rule, d_scratch_, scratch_stride_)) return -3;
	nbands_ = jobs.nbands; total_segs_ = (int)jobs.segjobs.size(); tok_per_frame_ = jobs.tok_per_frame;
	HIPCHK(hipMalloc(&d_bands_, jobs.bands.size() * sizeof(dev::EntBandJob)));
	HIPCHK(hipMemcpy(d_bands_, jobs.bands.data(), jobs.bands.size() * sizeof(dev::EntBandJob), hipMemcpyHostToDevice));
	HIPCHK(hipMalloc(&d_segband_, jobs.segjobs.size() * sizeof(dev::EntSegJob)));
	HIPCHK(hipMemcpy(d_segband_, jobs.segjobs.data(), jobs.segjobs.size() * sizeof(dev::EntSegJob), hipMemcpyHostToDevice));
	HIPCHK(hipMalloc(&d_segs_, jobs.segjobs.size() * sizeof(dev::EntSegState)));
	HIPCHK(hipMalloc(&d_tokens_, jobs.tok_per_frame * (size_t)n_ * sizeof(uint32_t)));      // token lists and finished bit strings: worst case one per coefficient, only the used part is ever touched
	HIPCHK(hipMalloc(&d_bandstate_, jobs.bands.size() * sizeof(dev::EntBandState)));
	static_assert((int)kBlockChunkCols == (int)dev::FWD_CHUNK_COLS_ENT, "one chunk geometry");
	if (lists) {
		int mask_base[kMaxChannels][kNumBands];
		masks_per_frame_ = (size_t)block_list_layout(plan, mask_base);
		HIPCHK(hipMalloc(&d_blocks_, stride * 2 * (size_t)n_));
		HIPCHK(hipMalloc((void **)&d_masks_, masks_per_frame_ * 8 * (size_t)n_ + 64));      // (+ spare entries: the inverse kernel fetches the masks of two chunks at a time)
		HIPCHK(hipMemset(d_masks_, 0, masks_per_frame_ * 8 * (size_t)n_ + 64));
	}
	HIPCHK(hipHostMalloc((void **)&h_samples_, cap_ * n_, hipHostMallocPortable));
	HIPCHK(hipMalloc((void **)&d_sizes_, sizeof(uint32_t) * 2 * n_));                   // [n] sample sizes, [n] peak flags
	HIPCHK(hipHostMalloc((void **)&h_sizes_, sizeof(uint32_t) * 2 * n_, hipHostMallocPortable));
	memset(h_sizes_, 0, sizeof(uint32_t) * 2 * n_);
	// the samples, densely: every one at its 64-byte aligned offset (none is longer than cap_, a multiple of 256) + the rest of the last 256-byte window a parser of the
	// last sample's tags may fetch (k_dec_parse)
	HIPCHK(hipMalloc((void **)&d_packed_, cap_ * n_ + 256));
	HIPCHK(hipMalloc((void **)&d_offsets_, sizeof(uint32_t) * (n_ + 1)));
	HIPCHK(hipHostMalloc((void **)&h_offsets_, sizeof(uint32_t) * (n_ + 1), hipHostMallocPortable));
	memset(h_offsets_, 0, sizeof(uint32_t) * (n_ + 1));
	HIPCHK(hipMalloc((void **)&d_tmpl_, (size_t)kEntTmplStride * n_));
	HIPCHK(hipHostMalloc((void **)&h_tmpl_, (size_t)kEntTmplStride * n_, hipHostMallocPortable));
	memset(h_tmpl_, 0, (size_t)kEntTmplStride * n_);
	HIPCHK(hipMalloc(&d_frames_, n_ * sizeof(dev::EntFrameJob)));
	HIPCHK(hipHostMalloc((void **)&host_->frames, n_ * sizeof(dev::EntFrameJob), hipHostMallocPortable));
	for (int f = 0; f < n_; f++) { SampleHeaderInfo h = hdr0; h.frame_number = (uint32_t)f + 1; if ((rc = set_frame_header(f, h))) return rc; }
	for (void *&e : ev_) HIPCHK(hipEventCreate((hipEvent_t *)&e));
	for (void *&e : ev2_) HIPCHK(hipEventCreate((hipEvent_t *)&e));
	// (the second stream: used with eight frames or more -- the level-1 count beside the level-2 / 3 transforms --; the C ABI's handles create it nevertheless:
	// cfhd_entropy_gpu.h device_streams_lean)
	if (n_ >= 8 || !device_streams_are_lean()) HIPCHK((hipError_t)device_stream_create(&stream2_));
	return 0;
}

int GpuEntropyEncoder::set_frame_header(int f, const SampleHeaderInfo &hdr)
{
	if (f < 0 || f >= n_) return -1;
	SampleTemplate &t = tmpl_[f];
	build_template(hdr, &t);
	if (!ent_fill_frame_block(host_->geom, t, f, host_->jobs, d_coeffs_ + (size_t)f * coeff_stride_, h_tmpl_ + (size_t)kEntTmplStride * f)) return -4;
	host_->frames[f] = ent_frame_job(t, d_tmpl_ + (size_t)kEntTmplStride * f, d_packed_, (uint32_t)cap_, d_sizes_ + f, d_sizes_ + n_ + f, d_offsets_ + f);
	dirty_ = true;
	return 0;
}

int GpuEntropyEncoder::launch(int first, int count)
{
	if (first < 0 || count < 1 || first + count > n_) return -1;
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	if (dirty_) {
		HIPCHK(hipMemcpyAsync(d_tmpl_, h_tmpl_, (size_t)kEntTmplStride * n_, hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d_frames_, host_->frames, n_ * sizeof(dev::EntFrameJob), hipMemcpyHostToDevice, st));
		dirty_ = false;
	}
	const dev::EntTables *T = (const dev::EntTables *)d_tables_;
	const dev::EntBatchGeom geom = { total_segs_ / n_, nbands_, coeff_stride_, tok_per_frame_ };
	const int act = count, segs_per_frame = total_segs_ / n_, total_segs = segs_per_frame * act;      // frames first .. first + act - 1 (set_active: 0 .. act-1)
	const dev::EntFrameJob *frames = (const dev::EntFrameJob *)d_frames_ + first;
	(void)hipGetLastError();
	HIPCHK(hipEventRecord((hipEvent_t)ev_[0], st));
#ifdef CFHD_AMD_PROBES
	const int count_probe = []{ const char *e = getenv("CFHD_AMD_COUNT_PROBE"); return e ? atoi(e) : 0; }();
#else
	const int count_probe = 0;
#endif
	const dev::EntBlockLists lists = { (const uint4 *)d_blocks_, d_masks_, d_coeffs_, masks_per_frame_ };
	auto count_range = [&](hipStream_t s, int lo, int n, bool level1 = false, const dev::EntBatchGeom *other = nullptr) {
		const dev::EntBatchGeom &g = other ? *other : geom;      // (other: the segments that read the scratch buffer)
		const int total = n * act;
		if (level1 && use_blocks_)
			dev::k_ent_count_blocks<<<(total + dev::ENT_WAVES - 1) / dev::ENT_WAVES, dev::ENT_THREADS, 0, s>>>((const dev::EntSegJob *)d_segband_, g, total, (dev::EntSegState *)d_segs_, T,
			                                                                                                 d_sizes_ + n_, (uint32_t *)d_tokens_, lo, n, lists, first);
		else
			dev::k_ent_count<<<(total + dev::ENT_WAVES - 1) / dev::ENT_WAVES, dev::ENT_THREADS, 0, s>>>((const dev::EntSegJob *)d_segband_, g, total, (dev::EntSegState *)d_segs_, T,
			                                                                                          d_sizes_ + n_, (uint32_t *)d_tokens_, lo, n, count_probe, first);
	};
	// CFHD_AMD_COUNT_SPLIT=0: (A/B) the level-1 bands counted on the main stream behind the level-2 / level-3 transforms instead of beside them
	static const bool split_on = [] { const char *e = getenv("CFHD_AMD_COUNT_SPLIT"); return !(e && atoi(e) == 0); }();
	split_ = split_on && ev_level1_ && stream2_ && !host_->jobs.ranges_l1.empty() && act >= 8;      // (a single frame gains nothing from six launches instead of one)
	serial_split_ = split_ && stream2_ == stream_;      // (a pass whose streams are one, cfhd_batch.cpp StreamScope: the same launches in a row, timed apart)
	// the level-1 bands on the second stream as soon as the level-1 transform is done; the bands of levels 2 and 3 on the main stream, behind their transforms; the scan waits for both
	hipStream_t s1 = split_ ? (hipStream_t)stream2_ : st;
	if (s1 != st) HIPCHK(hipStreamWaitEvent(s1, (hipEvent_t)ev_level1_, 0));
	// the peak flags are raised by the difference-coded band only, a level-1 band: cleared on the stream that counts it
	if (peak_flags_in_use()) HIPCHK(hipMemsetAsync(d_sizes_ + n_ + first, 0, sizeof(uint32_t) * (first ? act : n_), s1));
	// subband 7 in two passes: the two planes of every group and channel in one launch, behind the transforms and the division on the main stream; their segments are
	// counted apart from the others, with the scratch buffer's stride between the groups -- so a pass over such groups always counts range by range
	const std::vector<std::pair<int, int>> &scratch_ranges = host_->jobs.ranges_scratch;
	const dev::EntBatchGeom geom_scratch = { geom.segs_per_frame, geom.bands_per_frame, scratch_stride_, geom.tok_per_frame };
	dev::EntSplitJob sj;
	// (a window: the kernel numbers the groups from blockIdx.y = 0, so its job starts at the window's first pyramid and the window's first planes)
	if (!scratch_ranges.empty() && !ent_split_job(gplan_, d_coeffs_ + (size_t)first * coeff_stride_, coeff_stride_, d_scratch_ + (size_t)first * scratch_stride_, &sj)) return -3;
	auto count_scratch = [&] {      // (on the main stream, inside the span kernel_ms(0) times)
		if (scratch_ranges.empty()) return;
		uint32_t longest = 0;
		for (int c = 0; c < 3; c++) longest = sj.band[c].n > longest ? sj.band[c].n : longest;
		dev::k_ent_split_two_pass<<<dim3((longest / 8 + dev::ENT_THREADS - 1) / dev::ENT_THREADS, 3u * (unsigned)act), dev::ENT_THREADS, 0, st>>>(sj);
		for (const auto &r : scratch_ranges) count_range(st, r.first, r.second, false, &geom_scratch);
	};
	if (split_) {
		HIPCHK(hipEventRecord((hipEvent_t)ev2_[0], s1));
		for (const auto &r : host_->jobs.ranges_l1) count_range(s1, r.first, r.second, true);
		HIPCHK(hipEventRecord((hipEvent_t)ev2_[1], s1));
		count_scratch();
		for (const auto &r : host_->jobs.ranges_rest) count_range(st, r.first, r.second);
		HIPCHK(hipEventRecord((hipEvent_t)ev2_[2], st));
		if (s1 != st) HIPCHK(hipStreamWaitEvent(st, (hipEvent_t)ev2_[1], 0));
	} else if (use_blocks_ || !scratch_ranges.empty()) {
		count_scratch();
		for (const auto &r : host_->jobs.ranges_l1) count_range(st, r.first, r.second, true);
		for (const auto &r : host_->jobs.ranges_rest) count_range(st, r.first, r.second);
	} else count_range(st, 0, total_segs_ / n_);
	HIPCHK(hipEventRecord((hipEvent_t)ev_[1], st));
	// (a band job names its segments by their numbers in the whole batch: the window's bands and their states start first * nbands_ in)
	dev::k_ent_scan<<<nbands_ * act, dev::ENT_THREADS, 0, st>>>((const dev::EntBandJob *)d_bands_ + (size_t)first * nbands_, (dev::EntSegState *)d_segs_, (dev::EntBandState *)d_bandstate_ + (size_t)first * nbands_, T);
	HIPCHK(hipEventRecord((hipEvent_t)ev_[2], st));
	// every sample's size and its place in the dense buffer follow from what the scan left: nothing is written anywhere else, nothing is copied afterwards
	dev::k_ent_sizes<<<(act + dev::ENT_WAVES - 1) / dev::ENT_WAVES, dev::ENT_THREADS, 0, st>>>(frames, act, (const dev::EntBandState *)d_bandstate_);
	// (the offsets of all first + act frames: the sizes in front of the window are final, so their offsets come out as they were)
	dev::k_ent_pack_offsets<<<1, dev::ENT_THREADS, 0, st>>>(d_sizes_, first + act, d_offsets_);
	// workgroups per frame: enough to fill the chip for short batches of large frames, at least the 8 that 512 1080p frames were tuned with
	const unsigned layout_parts = act >= 256 ? 8u : (unsigned)((2048 + act - 1) / act > 256 ? 256 : (2048 + act - 1) / act);
	dev::k_ent_layout<<<dim3((unsigned)act, layout_parts), dev::ENT_THREADS, 0, st>>>(frames, (const dev::EntBandJob *)d_bands_, (dev::EntSegState *)d_segs_,
	                                                  (dev::EntBandState *)d_bandstate_, T);
	HIPCHK(hipEventRecord((hipEvent_t)ev_[3], st));
	// the values of the peak tables (interlaced plans: the difference-coded bands; a wave looks at a segment's record and leaves unless the segment has peaks)
	{
		dev::EntPeakHoles which; which.n = 0;
		for (size_t h = 0; h < tmpl_[0].holes.size() && which.n < 7; h++) if (tmpl_[0].holes[h].kind == 2) which.hole[which.n++] = (int)h;
		if (which.n) dev::k_ent_peaks<<<dim3(act >= 64 ? 4u : 32u, (unsigned)which.n, (unsigned)act), dev::ENT_THREADS, 0, st>>>(frames, which, (const dev::EntBandJob *)d_bands_,
		                                                  (const dev::EntSegJob *)d_segband_, geom, (const dev::EntSegState *)d_segs_, (const dev::EntBandState *)d_bandstate_);
	}
#ifdef CFHD_AMD_PROBES
	const int emit_probe = []{ const char *e = getenv("CFHD_AMD_EMIT_PROBE"); return e ? atoi(e) : 0; }();
#else
	const int emit_probe = 0;
#endif
	dev::k_ent_emit<<<(total_segs + dev::ENT_WAVES * dev::ENT_EMIT_SEGS - 1) / (dev::ENT_WAVES * dev::ENT_EMIT_SEGS), dev::ENT_THREADS, 0, st>>>(total_segs, (const dev::EntSegState *)d_segs_ + (size_t)first * segs_per_frame,
	                                                          T, (const uint32_t *)d_tokens_, emit_probe);      // (a segment's record names its tokens' place itself; the window's first segment opens a band)
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord((hipEvent_t)ev_[4], st));
	timed_ = true;
	return 0;
}

float GpuEntropyEncoder::kernel_ms(int k)
{
	float ms = 0;
	if (!timed_ || k < 0 || k > 4) return 0;
	if (k == 4) {                                        // the level-1 part of k_ent_count on the second stream (it runs beside the level-2 / level-3 transforms: its own events)
		if (!split_ || hipEventElapsedTime(&ms, (hipEvent_t)ev2_[0], (hipEvent_t)ev2_[1]) != hipSuccess) { (void)hipGetLastError(); return 0; }
		return ms;
	}
	void *end = (k == 0 && split_) ? ev2_[2] : ev_[k + 1];      // (the main stream's own launches, not its wait for the second stream)
	void *begin = (k == 0 && serial_split_) ? ev2_[1] : ev_[k];   // (one stream: the level-1 count ran in front, between ev2_[0] and ev2_[1])
	if (hipEventElapsedTime(&ms, (hipEvent_t)begin, (hipEvent_t)end) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return ms;
}

int GpuEntropyEncoder::fetch_sizes()
{
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	HIPCHK(hipMemcpyAsync(h_sizes_, d_sizes_, sizeof(uint32_t) * 2 * n_, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return 0;
}

int GpuEntropyEncoder::download() { const int rc = download_queue(); return rc ? rc : download_finish(); }      // (frames 0 .. active - 1)

// The part of download() that can be queued behind the kernels without the host: sizes and offsets on their way to the host, the samples -- written densely in HBM by
// launch() -- behind them.
int GpuEntropyEncoder::download_queue(int first, int count)
{
	if (first < 0 || count < 1 || first + count > n_) return -1;
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	// one copy out of HBM (SDMA engine when the runtime has it enabled; the kernels storing straight into the pinned host buffer measured slower in round 2)
	const int act = first + count;                       // (the sizes and offsets of the frames in front of a window travel again: they are what they were)
	HIPCHK(hipMemcpyAsync(h_sizes_, d_sizes_, sizeof(uint32_t) * 2 * n_, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(h_offsets_, d_offsets_, sizeof(uint32_t) * (act + 1), hipMemcpyDeviceToHost, st));
	// The copy of the sample bytes needs their number, which the host learns when the sizes arrive (download_finish()).  A pass that is queued as a whole
	// (cfhd_amd_batch_submit) would start that copy only when its result is collected, a step or two later; so the copy goes out now, sized by what the last pass of this
	// many frames produced plus a margin, and download_finish() adds the remainder if this pass turned out larger (consecutive passes of a sequence differ by a few percent).
	copied_ahead_ = 0;
	if (expect_bytes_ && expect_frames_ == act && !first) {
		copied_ahead_ = expect_bytes_ < cap_ * (size_t)act ? expect_bytes_ : cap_ * (size_t)act;
		HIPCHK(hipMemcpyAsync(h_samples_, d_packed_, copied_ahead_, hipMemcpyDeviceToHost, st));
	}
	return 0;
}

// ... and the part that needs the sizes: waits for the stream, then queues the one copy of all sample bytes (wait on the stream afterwards).
int GpuEntropyEncoder::download_finish(int first, int count)
{
	if (first < 0 || count < 1 || first + count > n_) return -1;
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	const int act = first + count;
	HIPCHK(hipStreamSynchronize(st));
	const size_t total = h_offsets_[act];
	if (first) copied_ahead_ = h_offsets_[first];        // (a window: the samples in front of it are on the host already, and unchanged)
	if (total > copied_ahead_) HIPCHK(hipMemcpyAsync(h_samples_ + copied_ahead_, d_packed_ + copied_ahead_, total - copied_ahead_, hipMemcpyDeviceToHost, st));
	expect_bytes_ = speculative_download_ ? ((total + total / 32 + 4095) & ~(size_t)4095) : 0; expect_frames_ = act;
	return 0;
}

struct GpuEntropyDecoder::Host {
	std::vector<std::vector<dev::DecBandJob>> bands;      // per frame
	std::vector<std::vector<dev::DecLowpassJob>> lows;
	std::vector<size_t> host_bytes;                       // bytes to copy H2D per frame (0: sample already in HBM)
	std::vector<std::vector<dev::DecDiffJob>> diffs;     // per frame: the difference-coded band of every channel (interlaced samples)
	dev::DecBandJob *flat_bands = nullptr; dev::DecLowpassJob *flat_lows = nullptr; dev::DecDiffJob *flat_diffs = nullptr;   // pinned
	dev::DecPlan plan;                                    // the slots of the job tables (dec_build_plan): fixed by prepare()
};

enum { kLowLatencyFrames = 32 };     // up to here k_dec_bands_par_ll: measured 0.22 vs 0.37 ms for one 1080p frame, break-even near 64 frames
static DecBackend par_backend(int nframes) { return nframes <= kLowLatencyFrames ? DecBackend::ParLowLatency : DecBackend::Par; }

GpuEntropyDecoder::GpuEntropyDecoder() : host_(new Host) {}
GpuEntropyDecoder::~GpuEntropyDecoder() { release(); delete host_; }

void GpuEntropyDecoder::release()
{
	(void)hipSetDevice(device_);
	void *dev[] = { d_samples_, d_tables_, d_bandjobs_, d_lowjobs_, d_errors_, d_plan_, d_idx_tables_, d_entries_, d_recs_, d_chunk_base_, d_chunk_job_, d_sums_, d_counters_, d_tile_start_, d_stats_, d_repair_, d_alts_, d_reindex_, d_diffjobs_, d_alt_entries_, d_masks_ };
	d_masks_ = nullptr; masks_per_frame_ = 0; use_blocks_ = false; blocks_written_ = false;
	for (void *p : dev) if (p) (void)hipFree(p);
	d_idx_tables_ = d_entries_ = d_recs_ = d_chunk_base_ = d_chunk_job_ = d_sums_ = d_counters_ = d_tile_start_ = d_stats_ = d_repair_ = d_alts_ = d_reindex_ = d_diffjobs_ = d_alt_entries_ = nullptr;
	if (h_chunk_job_) (void)hipHostFree(h_chunk_job_);
	if (h_counters_) (void)hipHostFree(h_counters_);
	h_chunk_job_ = nullptr; h_counters_ = nullptr;
	if (h_samples_) (void)hipHostFree(h_samples_);
	if (h_errors_) (void)hipHostFree(h_errors_);
	if (host_->flat_bands) { (void)hipHostFree(host_->flat_bands); host_->flat_bands = nullptr; }
	if (host_->flat_lows) { (void)hipHostFree(host_->flat_lows); host_->flat_lows = nullptr; }
	if (host_->flat_diffs) { (void)hipHostFree(host_->flat_diffs); host_->flat_diffs = nullptr; }
	for (void *&e : ev_) if (e) { (void)hipEventDestroy((hipEvent_t)e); e = nullptr; }
	if (ev_l23_) { (void)hipEventDestroy((hipEvent_t)ev_l23_); ev_l23_ = nullptr; }
	if (ev_low_) { (void)hipEventDestroy((hipEvent_t)ev_low_); ev_low_ = nullptr; }
	timed_ = false;
	d_samples_ = h_samples_ = nullptr; d_tables_ = d_bandjobs_ = d_lowjobs_ = d_plan_ = nullptr; d_errors_ = h_errors_ = nullptr; n_ = 0; ext_samples_ = nullptr;
}

int GpuEntropyDecoder::prepare(const FramePlan &plan, int nframes, int16_t *d_coeffs, size_t stride, size_t sample_cap, int out_kind, void *stream)
{
	int rc = device_init();
	if (rc) return rc;
	release();
	device_ = device_current(); (void)hipSetDevice(device_);
	plan_ = plan; n_ = nframes; cap_ = (sample_cap + 255) & ~(size_t)255; stream_ = stream; d_coeffs_ = d_coeffs; coeff_stride_ = stride; out_kind_ = out_kind;
	std::vector<uint32_t> t = build_dec_tables(1);
	HIPCHK(hipMalloc(&d_tables_, t.size() * 4));
	HIPCHK(hipMemcpy(d_tables_, t.data(), t.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMalloc((void **)&d_samples_, cap_ * n_));
	HIPCHK(hipHostMalloc((void **)&h_samples_, cap_ * n_, hipHostMallocPortable));
	const size_t max_bands = (size_t)n_ * kMaxChannels * 9, max_lows = (size_t)n_ * kMaxChannels;
	HIPCHK(hipMalloc(&d_bandjobs_, max_bands * sizeof(dev::DecBandJob)));
	HIPCHK(hipMalloc(&d_lowjobs_, max_lows * sizeof(dev::DecLowpassJob)));
	HIPCHK(hipHostMalloc((void **)&host_->flat_bands, max_bands * sizeof(dev::DecBandJob), hipHostMallocPortable));
	HIPCHK(hipHostMalloc((void **)&host_->flat_lows, max_lows * sizeof(dev::DecLowpassJob), hipHostMallocPortable));
	HIPCHK(hipMalloc(&d_diffjobs_, max_lows * sizeof(dev::DecDiffJob)));
	HIPCHK(hipHostMalloc((void **)&host_->flat_diffs, max_lows * sizeof(dev::DecDiffJob), hipHostMallocPortable));
	HIPCHK(hipMalloc((void **)&d_errors_, sizeof(int)));
	HIPCHK(hipHostMalloc((void **)&h_errors_, sizeof(int), hipHostMallocPortable));
	*h_errors_ = 0;
	// the band decoder, chosen here and nowhere else.  CFHD_AMD_DEC=lane / par: (A/B) the round-1 kernels -- par in its latency shape for few frames (the launch lasts as
	// long as the longest band's serial steps), in its throughput shape for many
	const char *be = getenv("CFHD_AMD_DEC");
	backend_ = be && strcmp(be, "lane") == 0 ? DecBackend::Lane : be && strcmp(be, "par") == 0 ? par_backend(n_) : DecBackend::ChunkIndexed;
	dev::DecPlan &dp = host_->plan;
	dec_build_plan(plan, out_kind, &dp);
	if (chunk_indexed()) {
		dev::DecIdxTables *it = new dev::DecIdxTables;
		const bool ok = build_dec_index_tables(1, it);
		if (ok) { hipError_t e = hipMalloc(&d_idx_tables_, sizeof(*it)); if (e == hipSuccess) e = hipMemcpy(d_idx_tables_, it, sizeof(*it), hipMemcpyHostToDevice); if (e != hipSuccess) { delete it; return g_fail(e, "decoder tables"); } }
		delete it;
		if (!ok) return -6;
		// chunk arrays for the worst case: every frame's sample as long as its slot, every band with a partial chunk
		const size_t per_frame = cap_ / dev::DX_CHUNK_BYTES + (size_t)kMaxChannels * 9 + 1;
		if (per_frame * (size_t)n_ >= ((size_t)1 << 31) / dev::DX_ENTRY_STRIDE * 8) return -5;
		max_chunks_ = (uint32_t)(per_frame * (size_t)n_);
		HIPCHK(hipMalloc(&d_entries_, (size_t)max_chunks_ * dev::DX_ENTRY_STRIDE * 4));
		HIPCHK(hipMalloc(&d_recs_, (size_t)max_chunks_ * sizeof(dev::DxChunkRec)));
		HIPCHK(hipMalloc(&d_chunk_base_, (size_t)max_chunks_ * 4));
		HIPCHK(hipMalloc(&d_chunk_job_, (size_t)max_chunks_ * sizeof(dev::DxChunkDesc)));
		HIPCHK(hipMalloc(&d_sums_, max_bands * sizeof(dev::DxBandSum)));
		HIPCHK(hipMalloc(&d_counters_, 32));          // [0] chunks, [1] bands to repair, [2] chunks to re-index, [3] alternate-entry slots taken, [4] next chunk of k_dec_index
		HIPCHK(hipMalloc(&d_repair_, max_bands * 4));
		HIPCHK(hipMalloc(&d_alts_, (size_t)max_chunks_ * sizeof(dev::DxChunkAlt)));
		HIPCHK(hipMalloc(&d_reindex_, (size_t)max_chunks_ * sizeof(dev::DxReindex)));
		alt_slots_ = max_chunks_ / 8 > 64u ? max_chunks_ / 8 : 64u;          // entries of the extra candidates of chunks without a unique alignment (a few per cent of the chunks)
		HIPCHK(hipMalloc(&d_alt_entries_, (size_t)alt_slots_ * dev::DX_ENTRY_STRIDE * 4));
		HIPCHK(hipMalloc(&d_tile_start_, ((size_t)dx_tile_plan(plan, dp, n_, false).total + 1) * sizeof(dev::DxTileDesc)));      // one record per tile (k_dec_tile_index)
		const char *se = getenv("CFHD_AMD_DX_STATS");
		if (se && atoi(se)) { HIPCHK(hipMalloc(&d_stats_, 64)); HIPCHK(hipMemset(d_stats_, 0, 64)); }
		HIPCHK(hipHostMalloc((void **)&h_chunk_job_, (size_t)max_chunks_ * sizeof(dev::DxChunkDesc), hipHostMallocPortable));
		HIPCHK(hipHostMalloc((void **)&h_counters_, 32, hipHostMallocPortable));
		int cus = 256;
		(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_current());
		// workgroups that fit a CU at once: k_dec_index 31 KB of LDS each, k_dec_tiles its tables (22.5 KB) + the image of a tile
		grid_index_[0] = cus * 5; grid_tiles_[0] = cus * (int)((160 * 1024) / (sizeof(uint2) * (1 << dev::DX_KM) + sizeof(uint32_t) * (dev::DX_LONG11_MAX + dev::DX_TILE_WORDS)));
		// The shared shapes, for launches beside other passes in flight (launch_dx): both kernels wait on LDS latency rather than on instruction issue, and resident
		// for a whole launch with every slot taken they leave the VALU-bound kernels of the other passes no LDS to start in.  Measured under four passes in flight
		// (profiles/dx_shared_grids_ab.txt).  CFHD_AMD_DX_SHARED=0: the solo shapes for every launch.
		grid_index_[1] = cus * kDxSharedIndexPerCu; grid_tiles_[1] = cus * kDxSharedTilesPerCu;
		if (grid_index_[1] > grid_index_[0]) grid_index_[1] = grid_index_[0];
		if (grid_tiles_[1] > grid_tiles_[0]) grid_tiles_[1] = grid_tiles_[0];
		if (const char *e = getenv("CFHD_AMD_DX_SHARED")) if (atoi(e) == 0) { grid_index_[1] = grid_index_[0]; grid_tiles_[1] = grid_tiles_[0]; }
		// one shape for every launch (sweeps: tools/dx_index_sweep.sh, tools/dx_tile_sweep.sh; tests: a workgroup that decodes chunk after chunk, tile after tile)
		if (const char *e = getenv("CFHD_AMD_DX_GRID_INDEX")) if (atoi(e) > 0) grid_index_[0] = grid_index_[1] = atoi(e);
		if (const char *e = getenv("CFHD_AMD_DX_GRID_TILES")) if (atoi(e) > 0) grid_tiles_[0] = grid_tiles_[1] = atoi(e);
		for (int k = 0; k < 2; k++) { if (grid_index_[k] < 1) grid_index_[k] = 1; if (grid_tiles_[k] < 1) grid_tiles_[k] = 1; }
	}
	HIPCHK(hipMalloc(&d_plan_, sizeof(dp)));
	HIPCHK(hipMemcpy(d_plan_, &dp, sizeof(dp), hipMemcpyHostToDevice));
	// chunk masks of the level-1 bands as block lists (cfhd_core.h dec_block_list_layout): for 4:2:2 frames, whose last level has a strip kernel that gathers them
	if (chunk_indexed() && plan.encoded_format == ENC_YUV422 && plan.num_channels == 3) {
		int mask_base[kMaxChannels][kNumBands];
		masks_per_frame_ = (size_t)dec_block_list_layout(plan, mask_base);
		HIPCHK(hipMalloc((void **)&d_masks_, masks_per_frame_ * 8 * (size_t)n_));
	}
	host_->bands.assign(n_, {}); host_->lows.assign(n_, {}); host_->diffs.assign(n_, {}); host_->host_bytes.assign(n_, 0);
	for (void *&e : ev_) HIPCHK(hipEventCreate((hipEvent_t *)&e));
	HIPCHK(hipEventCreate((hipEvent_t *)&ev_l23_));
	HIPCHK(hipEventCreate((hipEvent_t *)&ev_low_));
	return 0;
}

int GpuEntropyDecoder::set_samples_device(const uint8_t *d_samples, size_t stride_bytes, const uint32_t *d_sizes, const uint32_t *d_offsets)
{
	// k_dec_parse reads windows of 256 bytes counted from the sample's start, longword by longword: a slot must extend to the window that holds its last tag, the buffer
	// behind dense samples to the last sample's (every other window ends inside the next sample)
	if (!d_samples || !d_sizes || ((uintptr_t)d_samples & 255) || (!d_offsets && (stride_bytes & 255))) return -1;
	ext_samples_ = d_samples; ext_stride_ = stride_bytes; ext_sizes_ = d_sizes; ext_offsets_ = d_offsets;
	return 0;
}

int GpuEntropyDecoder::set_sample_host(int i, const uint8_t *sample, size_t size)
{
	if (i < 0 || i >= n_ || size > cap_) return -1;
	memcpy(h_samples_ + cap_ * i, sample, size);
	int rc = set_sample_device(i, d_samples_ + cap_ * i, sample, size);
	if (rc == 0) host_->host_bytes[i] = (size + 3) & ~(size_t)3;
	return rc;
}

int GpuEntropyDecoder::set_sample_device(int i, const uint8_t *d_sample, const uint8_t *host_copy, size_t size)
{
	if (i < 0 || i >= n_) return -1;
	ext_samples_ = nullptr;
	ParsedSample ps;
	if (parse_sample(host_copy, size, &ps) != 0) return -2;
	if (ps.width != plan_.width || ps.display_height != plan_.display_height || ps.encoded_format != plan_.encoded_format || ps.num_channels != plan_.num_channels) return -3;
	host_->bands[i].clear(); host_->lows[i].clear(); host_->host_bytes[i] = 0;
	if (chunk_indexed()) {
		// rows of the [slot][frame] job table, by slot
		const dev::DecPlan &dp = host_->plan;
		host_->bands[i].assign((size_t)dp.bands_per_frame, dev::DecBandJob());
		host_->lows[i].assign((size_t)plan_.num_channels, dev::DecLowpassJob());
		host_->diffs[i].assign((size_t)plan_.num_channels, dev::DecDiffJob());
		if (!dx_build_jobs(ps, plan_, dp, d_sample, d_coeffs_ + (size_t)i * coeff_stride_, out_kind_, 0, 1, host_->bands[i].data(), host_->lows[i].data(), skip_level1_,
		                   interlaced_ ? host_->diffs[i].data() : nullptr)) return -4;
		return 0;
	}
	if (interlaced_) return -4;                        // the round-1 kernels know one code set
	if (!dec_build_jobs(ps, plan_, d_sample, d_coeffs_ + (size_t)i * coeff_stride_, out_kind_, &host_->bands[i], &host_->lows[i], skip_level1_)) return -4;
	return 0;
}

// The host's job tables as the kernels read them.  Chunk-indexed decoder: [slot][frame] over the frames that carry samples (set_active), the chunks numbered here.
// Round-1 kernels: band-type major over the whole batch -- the 64 lanes of a wave (lane kernel) decode bands of similar length, and the workgroups of the parallel
// kernel start with the long bands (level-1 luma first) so that the short ones fill the tail of the launch.
int GpuEntropyDecoder::flatten_host_jobs(Pass *p)
{
	const int nch = plan_.num_channels;
	dev::DecBandJob *fb = host_->flat_bands; dev::DecLowpassJob *fl = host_->flat_lows;
	if (chunk_indexed()) {
		const int slots = host_->plan.bands_per_frame, act = active_frames();
		for (int f = 0; f < act; f++) {
			if ((int)host_->bands[f].size() != slots || (int)host_->lows[f].size() != nch) return -1;
			for (int s = 0; s < slots; s++) fb[(size_t)s * act + f] = host_->bands[f][s];
			for (int c = 0; c < nch; c++) fl[(size_t)f * nch + c] = host_->lows[f][c];
			if (interlaced_) { if ((int)host_->diffs[f].size() != nch) return -1; for (int c = 0; c < nch; c++) host_->flat_diffs[(size_t)f * nch + c] = host_->diffs[f][c]; }
		}
		std::vector<dev::DxChunkDesc> cj;
		const uint32_t nchunks = dx_number_chunks(fb, slots * act, &cj);
		if (nchunks > max_chunks_) return -5;
		memcpy(h_chunk_job_, cj.data(), cj.size() * sizeof(dev::DxChunkDesc));
		h_counters_[0] = nchunks; h_counters_[1] = 0; h_counters_[2] = 0; h_counters_[3] = 0; h_counters_[4] = 0;
		*p = Pass{ false, act, slots * act, act * nch, nchunks };
		return 0;
	}
	size_t nfb = 0, nfl = 0, per_frame = 0;
	for (int f = 0; f < n_; f++) per_frame = host_->bands[f].size() > per_frame ? host_->bands[f].size() : per_frame;
	for (size_t k = 0; k < per_frame; k++) for (int f = 0; f < n_; f++) if (k < host_->bands[f].size()) fb[nfb++] = host_->bands[f][k];
	for (int f = 0; f < n_; f++) for (const dev::DecLowpassJob &j : host_->lows[f]) fl[nfl++] = j;
	if (!nfb) return -1;
	if (backend_ != DecBackend::Lane) std::stable_sort(fb, fb + nfb, [](const dev::DecBandJob &a, const dev::DecBandJob &b) { return a.bytes > b.bytes; });
	else HIPCHK(hipMemset2DAsync(d_coeffs_, coeff_stride_ * 2, 0, (size_t)plan_.final_elems * 2, n_, (hipStream_t)stream_));   // the parallel kernel clears its own bands
	*p = Pass{ false, n_, (int)nfb, (int)nfl, 0u };
	return 0;
}

// The round-1 band kernels (the only place that names them): a lane per band, or a workgroup per band in its latency or its throughput shape.
void GpuEntropyDecoder::launch_round1(DecBackend backend, int nb)
{
	hipStream_t st = (hipStream_t)stream_;
	const dev::DecBandJob *jobs = (const dev::DecBandJob *)d_bandjobs_; const dev::DecTables *T = (const dev::DecTables *)d_tables_;
	if (backend == DecBackend::Lane) dev::k_dec_bands<<<(nb + dev::DEC_THREADS - 1) / dev::DEC_THREADS, dev::DEC_THREADS, 0, st>>>(jobs, nb, T, d_errors_);
	else if (backend == DecBackend::ParLowLatency) dev::k_dec_bands_par_ll<<<nb, dev::DECP_LL_THREADS, 0, st>>>(jobs, T, d_errors_);
	else dev::k_dec_bands_par<<<nb, dev::DECP_THREADS, 0, st>>>(jobs, T, d_errors_);
}

// One pass over the batch: the job tables (parsed on the GPU from device-resident samples, or uploaded with the host-parsed samples), the band decoder -- by default the
// chunk-indexed one, launch_dx --, the lowpass bands, the error flag on its way to the host.
int GpuEntropyDecoder::launch()
{
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	const int nch = plan_.num_channels;
	l23_split_ = false; blocks_written_ = false;
	// device-resident samples: the job tables have one row per band type (largest first), nframes wide, and the device numbers the chunks
	const int nd = active_frames();                      // (device-resident samples: all of them unless a short pass of the decode queue said otherwise)
	Pass p = { true, nd, nd * nch * 9, nd * nch, max_chunks_ };
	if (!ext_samples_) {
		if (chunk_indexed()) HIPCHK(hipStreamSynchronize(st));                    // the pinned tables of the previous launch may still be in flight
		const int rc = flatten_host_jobs(&p);
		if (rc) return rc;
	}
	HIPCHK(hipMemsetAsync(d_errors_, 0, sizeof(int), st));
	if (p.device_jobs) {
		(void)hipGetLastError();
		// CFHD_AMD_PARSE_EARLY=0: (A/B) the parser behind the finished payloads instead of beside k_ent_emit
		static const bool parse_early = [] { const char *e = getenv("CFHD_AMD_PARSE_EARLY"); return !(e && atoi(e) == 0); }();
		if (!parse_early && ev_payloads_) ev_headers_ = ev_payloads_;
		if (ev_headers_) HIPCHK(hipStreamWaitEvent(st, (hipEvent_t)ev_headers_, 0));
		HIPCHK(hipEventRecord((hipEvent_t)ev_[0], st));
		dev::k_dec_parse<<<nd, dev::DEC_PARSE_THREADS, 0, st>>>(ext_samples_, ext_stride_, ext_sizes_, nd,
			(const dev::DecPlan *)d_plan_, d_coeffs_, coeff_stride_, (dev::DecBandJob *)d_bandjobs_, (dev::DecLowpassJob *)d_lowjobs_, d_errors_,
			interlaced_ && chunk_indexed() ? (dev::DecDiffJob *)d_diffjobs_ : nullptr, ext_offsets_, d_verdicts_);
		parse_end_ = ev_payloads_ != nullptr;
		if (parse_end_) { HIPCHK(hipEventRecord((hipEvent_t)ev_[4], st)); HIPCHK(hipStreamWaitEvent(st, (hipEvent_t)ev_payloads_, 0)); }
		ev_headers_ = ev_payloads_ = nullptr;
	} else {
		parse_end_ = false;
		for (int f = 0; f < p.frames; f++)
			if (host_->host_bytes[f]) HIPCHK(hipMemcpyAsync(d_samples_ + cap_ * f, h_samples_ + cap_ * f, host_->host_bytes[f], hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d_bandjobs_, host_->flat_bands, (size_t)p.band_jobs * sizeof(dev::DecBandJob), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d_lowjobs_, host_->flat_lows, (size_t)p.lowpass_jobs * sizeof(dev::DecLowpassJob), hipMemcpyHostToDevice, st));
		if (chunk_indexed()) {
			if (interlaced_) HIPCHK(hipMemcpyAsync(d_diffjobs_, host_->flat_diffs, (size_t)p.lowpass_jobs * sizeof(dev::DecDiffJob), hipMemcpyHostToDevice, st));
			HIPCHK(hipMemcpyAsync(d_chunk_job_, h_chunk_job_, (size_t)p.chunks * sizeof(dev::DxChunkDesc), hipMemcpyHostToDevice, st));
			HIPCHK(hipMemcpyAsync(d_counters_, h_counters_, 20, hipMemcpyHostToDevice, st));
		}
		(void)hipGetLastError();
		HIPCHK(hipEventRecord((hipEvent_t)ev_[0], st));
	}
	HIPCHK(hipEventRecord((hipEvent_t)ev_[1], st));
	// (the lane kernel wants the pyramid cleared and its jobs from the host: device-resident samples go to the parallel one)
	const DecBackend round1 = p.device_jobs && backend_ == DecBackend::Lane ? par_backend(n_) : backend_;
	if (chunk_indexed()) { const int rc = launch_dx(p); if (rc) return rc; }
	else launch_round1(round1, p.band_jobs);
	HIPCHK(hipEventRecord((hipEvent_t)ev_[2], st));
	if (!l23_split_) dev::k_dec_lowpass<<<dim3(8, (unsigned)p.lowpass_jobs), 256, 0, st>>>((const dev::DecLowpassJob *)d_lowjobs_);      // (split: launched between the two tile passes)
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord((hipEvent_t)ev_[3], st));
	timed_ = true;
	HIPCHK(hipMemcpyAsync(h_errors_, d_errors_, sizeof(int), hipMemcpyDeviceToHost, st));
	return 0;
}

// The chunk-indexed decoder on the batch's stream.
int GpuEntropyDecoder::launch_dx(const Pass &p)
{
	hipStream_t st = (hipStream_t)stream_;
	dev::DecBandJob *jobs = (dev::DecBandJob *)d_bandjobs_;
	const dev::DecIdxTables *T = (const dev::DecIdxTables *)d_idx_tables_;
	const int njobs = p.band_jobs;
	const bool lists = use_blocks_ && d_masks_ && !skip_level1_;
	const dev::DxTilePlan tp = dx_tile_plan(plan_, host_->plan, p.frames, skip_level1_, lists, interlaced_);
	unsigned long long *const tmasks = lists ? d_masks_ : nullptr;
	blocks_written_ = lists;
	const char *spec_env = getenv("CFHD_AMD_DX_SPECULATE");
	const bool speculate = !(spec_env && atoi(spec_env) == 0);            // 0: every chunk goes through the repair path (tests)
	if (p.device_jobs) {
		// the repair and re-index lists, the alternate-entry slots and the chunk counter start at zero (the host path uploads zeroed counters); the chunks are numbered here
		HIPCHK(hipMemsetAsync((uint32_t *)d_counters_ + 1, 0, 16, st));
		dev::k_dec_plan<<<1, 1024, 0, st>>>(jobs, njobs, max_chunks_, (uint32_t *)d_counters_, d_errors_);
		dev::k_dec_plan_fill<<<(njobs + dev::DX_WAVES - 1) / dev::DX_WAVES, dev::DX_THREADS, 0, st>>>(jobs, njobs, (dev::DxChunkDesc *)d_chunk_job_, (const uint32_t *)d_counters_);
	}
	HIPCHK(hipEventRecord((hipEvent_t)ev_[7], st));         // (k_dec_index is timed by itself: kernel_ms(3); the plan in front of it: kernel_ms(6))
	// grid-stride kernels: as many workgroups as the chip holds at once, fewer when there is less work (k_dec_tiles: a workgroup per tile)
	// (the shared shapes when passes other than this decoder's own are in flight on the device: a hint read here, on the host, while the pass is queued.  device_
	// is the device the owner counts its pass on: a batch prepares its encoder and its decoder on one device)
	const int shape = device_passes_in_flight(device_) - (pass_counted_ ? 1 : 0) > 0 ? 1 : 0;
	int g1 = grid_index_[shape], g3 = grid_tiles_[shape];
	if ((uint32_t)g1 * dev::DX_WAVES > p.chunks) g1 = (int)((p.chunks + dev::DX_WAVES - 1) / dev::DX_WAVES);
	if ((uint32_t)g3 > tp.total) g3 = (int)tp.total;
	if (g1 < 1) g1 = 1;
	if (g3 < 1) g3 = 1;
	dev::k_dec_index<<<g1, dev::DX_THREADS, 0, st>>>((const dev::DxChunkDesc *)d_chunk_job_, (const uint32_t *)d_counters_, T, (uint32_t *)d_entries_, (dev::DxChunkRec *)d_recs_, (dev::DxChunkAlt *)d_alts_, speculate ? 1 : 0, (uint32_t *)d_stats_,
	                                                 (uint32_t *)d_alt_entries_, alt_slots_, (uint32_t *)d_counters_ + 3, (uint32_t *)d_counters_ + 4);
	HIPCHK(hipEventRecord((hipEvent_t)ev_[5], st));
	dev::k_dec_chain<<<(njobs + dev::DX_WAVES - 1) / dev::DX_WAVES, dev::DX_THREADS, 0, st>>>(jobs, njobs, (const dev::DxChunkRec *)d_recs_, (const dev::DxChunkAlt *)d_alts_, (uint32_t *)d_chunk_base_,
	                                                                                            (dev::DxBandSum *)d_sums_, d_errors_, (uint32_t *)d_repair_, (dev::DxReindex *)d_reindex_, (uint32_t *)d_counters_);
	const int small_grid = njobs < 256 ? (njobs + dev::DX_WAVES - 1) / dev::DX_WAVES : 64;
	dev::k_dec_repair<<<small_grid, dev::DX_THREADS, 0, st>>>(jobs, T, (uint32_t *)d_entries_, (dev::DxChunkRec *)d_recs_, (const dev::DxChunkAlt *)d_alts_, (uint32_t *)d_chunk_base_, (dev::DxBandSum *)d_sums_,
	                                                         d_errors_, (const uint32_t *)d_repair_, (dev::DxReindex *)d_reindex_, (uint32_t *)d_counters_, (uint32_t *)d_stats_);
	dev::k_dec_reindex<<<g1, dev::DX_THREADS, 0, st>>>(jobs, T, (uint32_t *)d_entries_, (const dev::DxReindex *)d_reindex_, (const uint32_t *)d_counters_, (uint32_t *)d_stats_,
	                                                   (const dev::DxChunkAlt *)d_alts_, (const uint32_t *)d_alt_entries_);
	dev::k_dec_tile_index<<<(tp.total + dev::DX_TILE_INDEX_TILES - 1) / dev::DX_TILE_INDEX_TILES, dev::DX_THREADS, 0, st>>>(jobs, tp, (const uint32_t *)d_entries_, (const uint32_t *)d_chunk_base_, (const dev::DxBandSum *)d_sums_,
	                                                                                                  (dev::DxTileDesc *)d_tile_start_, tmasks, (uint32_t)masks_per_frame_);
	HIPCHK(hipEventRecord((hipEvent_t)ev_[6], st));
	// Many frames: the tiles of the level-2 / level-3 bands (a quarter of them) and the lowpass bands first, an event behind them, then the level-1 tiles -- the caller
	// may run the inverse transforms of levels 3 and 2 on another stream beside the second launch (DecodeBatch::launch_inverse).  Off unless CFHD_AMD_TILES_SPLIT=1:
	// measured in round 3 (1080p, 512 frames), the step does not get shorter (48.1 k fps either way) -- k_dec_tiles is bound by instruction issue and owns its CUs' LDS,
	// the plane kernels beside it only stretch it from 1.67 to 2.25 ms.  (The same idea pays on the encoder side, where the kernel that shares the chip waits on memory.)
	const char *split_env = getenv("CFHD_AMD_TILES_SPLIT");
	l23_split_ = p.frames >= 8 && !skip_level1_ && tp.split > 0 && tp.split < tp.total && split_env && split_env[0] == '1';
	auto tile_pass = [&](const dev::DxTilePlan &t, int g) {
		dev::k_dec_tiles<dev::DX_TILE_THREADS><<<g < 1 ? 1 : g, dev::DX_TILE_THREADS, 0, st>>>((const dev::DxTileDesc *)d_tile_start_, t.first, t.total, T, (const uint32_t *)d_entries_, (const uint32_t *)d_chunk_base_);
	};
	if (l23_split_) {
		dev::DxTilePlan ta = tp, tb = tp;
		ta.total = tp.split; tb.first = tp.split;
		tile_pass(ta, (uint32_t)g3 > ta.total ? (int)ta.total : g3);
		HIPCHK(hipEventRecord((hipEvent_t)ev_low_, st));
		dev::k_dec_lowpass<<<dim3(8, (unsigned)p.lowpass_jobs), 256, 0, st>>>((const dev::DecLowpassJob *)d_lowjobs_);
		HIPCHK(hipEventRecord((hipEvent_t)ev_l23_, st));
		tile_pass(tb, (uint32_t)g3 > tb.total - tb.first ? (int)(tb.total - tb.first) : g3);
	} else tile_pass(tp, g3);
	if (interlaced_) {
		// the difference-coded band of every channel back to coefficients: a wave per row for the bands without a peak table, the workgroup-per-band
		// kernel of round 3 for the few that have one (measured against that kernel for all of them: profiles/r04_o_*)
		dev::k_dec_undiff_rows<<<dim3((unsigned)(p.frames * plan_.num_channels), 32), 64 * dev::DXR_WAVES, 0, st>>>((const dev::DecDiffJob *)d_diffjobs_);
		dev::k_dec_undiff<<<dim3((unsigned)(p.frames * plan_.num_channels), dev::DXU_SPLIT), dev::DXU_THREADS, 0, st>>>((const dev::DecDiffJob *)d_diffjobs_, d_errors_, 1);
	}
	HIPCHK(hipGetLastError());
	return 0;
}

int GpuEntropyDecoder::check() { return *h_errors_ ? -1 : 0; }

// CFHD_AMD_DX_STATS=1: counters of k_dec_index / k_dec_chain since prepare(): [0] rounds, [1] chunks indexed, [2] most rounds of a chunk, [3] chunks repaired,
// [4..15] lanes that restarted in round 0..10, 11+.  Synchronises the stream.
int GpuEntropyDecoder::stats(uint32_t out[16])
{
	(void)hipSetDevice(device_);
	memset(out, 0, 64);
	if (!d_stats_) return -1;
	HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
	HIPCHK(hipMemcpy(out, d_stats_, 64, hipMemcpyDeviceToHost));
	return 0;
}

float GpuEntropyDecoder::kernel_ms(int k)
{
	float ms = 0;
	if (k >= 3) {                                                // the chunk-indexed decoder's own kernels
		if (!timed_ || !chunk_indexed() || k > 6) return 0;
		// 3: k_dec_index, 4: k_dec_chain (+ repair, reindex, tile index), 5: k_dec_tiles, 6: k_dec_plan + k_dec_plan_fill (one workgroup that numbers the chunks: latency, not work)
		void *a = k == 3 ? ev_[7] : (k == 4 ? ev_[5] : (k == 5 ? ev_[6] : ev_[1])), *b = k == 3 ? ev_[5] : (k == 4 ? ev_[6] : (k == 5 ? ev_[2] : ev_[7]));
		if (hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b) != hipSuccess) { (void)hipGetLastError(); return 0; }
		if (k == 5 && l23_split_) {                          // k_dec_lowpass ran between the two tile passes: not part of k_dec_tiles
			float low = 0;
			if (hipEventElapsedTime(&low, (hipEvent_t)ev_low_, (hipEvent_t)ev_l23_) == hipSuccess) ms -= low; else (void)hipGetLastError();
		}
		return ms;
	}
	if (k == 2 && l23_split_ && timed_) {                        // k_dec_lowpass between the two tile passes
		if (hipEventElapsedTime(&ms, (hipEvent_t)ev_low_, (hipEvent_t)ev_l23_) != hipSuccess) { (void)hipGetLastError(); return 0; }
		return ms;
	}
	void *end = (k == 0 && parse_end_) ? ev_[4] : ev_[k + 1];      // the parser's own end, not the start of the band decoder that waited for the payloads
	if (!timed_ || k < 0 || k > 2 || hipEventElapsedTime(&ms, (hipEvent_t)ev_[k], (hipEvent_t)end) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return ms;
}

// =============================================================================================
// GpuGroupEntropyDecoder
// =============================================================================================
void GpuGroupEntropyDecoder::release()
{
	(void)hipSetDevice(device_);
	void *dev[] = { d_sample_, d_tables_, d_tables18_, d_bandjobs_, d_lowjobs_, d_diffjobs_, d_errors_ };
	for (void *p : dev) if (p) (void)hipFree(p);
	void *host[] = { h_sample_, h_bandjobs_, h_lowjobs_, h_diffjobs_, h_errors_ };
	for (void *p : host) if (p) (void)hipHostFree(p);
	d_sample_ = h_sample_ = nullptr; d_tables_ = d_tables18_ = d_bandjobs_ = d_lowjobs_ = d_diffjobs_ = h_bandjobs_ = h_lowjobs_ = h_diffjobs_ = nullptr; d_errors_ = h_errors_ = nullptr;
}

enum { kGroupBandJobs = 3 * 15, kGroupRawJobs = 3 * 2, kGroupDiffJobs = 3 * 2 };

int GpuGroupEntropyDecoder::prepare(const GopPlan &plan, int16_t *d_coeffs, size_t sample_cap, int out_kind, void *stream, int device)
{
	int rc = device_init();
	if (rc) return rc;
	release();
	device_ = device >= 0 ? device : device_current(); (void)hipSetDevice(device_);      // (the GPU the pyramid and the stream live on)
	plan_ = plan; d_coeffs_ = d_coeffs; cap_ = (sample_cap + 255) & ~(size_t)255; out_kind_ = out_kind; stream_ = stream;
	std::vector<uint32_t> t = build_dec_tables(1);
	HIPCHK(hipMalloc(&d_tables_, t.size() * 4));
	HIPCHK(hipMemcpy(d_tables_, t.data(), t.size() * 4, hipMemcpyHostToDevice));
	t = build_dec_tables(2);
	HIPCHK(hipMalloc(&d_tables18_, t.size() * 4));
	HIPCHK(hipMemcpy(d_tables18_, t.data(), t.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMalloc(&d_diffjobs_, kGroupDiffJobs * sizeof(dev::DecDiffJob)));
	HIPCHK(hipHostMalloc(&h_diffjobs_, kGroupDiffJobs * sizeof(dev::DecDiffJob), hipHostMallocPortable));
	HIPCHK(hipMalloc((void **)&d_sample_, cap_));
	HIPCHK(hipHostMalloc((void **)&h_sample_, cap_, hipHostMallocPortable));
	HIPCHK(hipMalloc(&d_bandjobs_, kGroupBandJobs * sizeof(dev::DecBandJob)));
	HIPCHK(hipMalloc(&d_lowjobs_, kGroupRawJobs * sizeof(dev::DecLowpassJob)));
	HIPCHK(hipHostMalloc(&h_bandjobs_, kGroupBandJobs * sizeof(dev::DecBandJob), hipHostMallocPortable));
	HIPCHK(hipHostMalloc(&h_lowjobs_, kGroupRawJobs * sizeof(dev::DecLowpassJob), hipHostMallocPortable));
	HIPCHK(hipMalloc((void **)&d_errors_, sizeof(int)));
	HIPCHK(hipHostMalloc((void **)&h_errors_, sizeof(int), hipHostMallocPortable));
	*h_errors_ = 0;
	return 0;
}

int GpuGroupEntropyDecoder::launch(const uint8_t *sample, size_t size, const ParsedGroup &pg)
{
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	if (size > cap_) return -1;
	HIPCHK(hipStreamSynchronize(st));                                       // the pinned sample / tables of the previous launch may still be in flight
	dev::DecBandJob *bj = (dev::DecBandJob *)h_bandjobs_; dev::DecLowpassJob *lj = (dev::DecLowpassJob *)h_lowjobs_; dev::DecDiffJob *dj = (dev::DecDiffJob *)h_diffjobs_;
	int nb = 0, nl = 0, nd = 0;
	for (int c = 0; c < 3; c++) {
		const GopChannel &ch = plan_.ch[c];
		const ParsedBand &lp = pg.lowpass[c];
		const GopWavelet &top = ch.w[5];
		if (!lp.present || lp.width != top.width || lp.height != top.height || (size_t)lp.offset + (size_t)top.width * top.height * 2 > size) return -2;
		// the bias the reference adds to the lowpass band while unpacking it: the group's of the requested output (group_lowpass_bias; decoder.c:12265 `num_frames == 2 ? 48 : 24`)
		lj[nl++] = dev::DecLowpassJob{ d_sample_ + lp.offset, d_coeffs_ + top.offset[0], top.width, top.height, top.pitch, group_lowpass_bias(top.width, out_kind_, c) };
		static const int coded[5] = { 5, 4, 3, 1, 0 };
		for (int k : coded) {
			const GopWavelet &wv = ch.w[k];
			for (int b = (k == 3 ? 0 : 1); b < 4; b++) {
				const ParsedBand &pb = pg.band[c][k][b];
				if (!pb.present || pb.width != wv.width || pb.height != wv.height || (pb.offset & 3) || (size_t)pb.offset + pb.bytes > size) return -2;
				if (pb.codebook == -2) return -3;                            // (coded in two passes, cfhd_gop.h: the host coder's)
				if (pb.codebook < 0) {                                       // raw 16-bit words (the lowpass band of the temporal highpass wavelet): signed, no bias
					if ((size_t)pb.bytes < (size_t)wv.width * wv.height * 2 || pb.quant != 1 || (wv.width & 1)) return -3;
					lj[nl++] = dev::DecLowpassJob{ d_sample_ + pb.offset, d_coeffs_ + wv.offset[0], wv.width, wv.height, wv.pitch, 0 };
					continue;
				}
				// the difference-coded bands of an interlaced group (band 2 of the two frame wavelets: subbands 12 and 15) come in code set 18, maybe with a peak table
				const bool diff = gop_band_is_difference_coded(plan_, k, b);
				if (pb.codebook != (diff ? 2 : 1) || pb.difference != diff || (wv.offset[b] & 7) || (wv.pitch & 7)) return -3;
				if (diff) {
					if (nd >= kGroupDiffJobs || wv.width > 16 * 256 || (pb.peak_level && (size_t)pb.peak_offset + 2 > size)) return -3;      // (k_dec_undiff: rows of up to DXU_MAX x DXU_THREADS coefficients)
					dj[nd++] = dev::DecDiffJob{ d_coeffs_ + wv.offset[b], wv.width, wv.height, wv.pitch, pb.peak_level ? d_sample_ + pb.peak_offset : nullptr,
					                            pb.peak_level ? (uint32_t)(size - pb.peak_offset) : 0u, pb.peak_level };
				}
				bj[nb++] = dev::DecBandJob{ d_sample_ + pb.offset, pb.bytes, d_coeffs_ + wv.offset[b], wv.height * wv.pitch, pb.quant, 0u, diff ? 1 : 0 };
			}
		}
	}
	if (nb != kGroupBandJobs || nl != kGroupRawJobs || nd != (plan_.interlaced ? kGroupDiffJobs : 0)) return -2;
	// the bands of code set 17 in front, those of code set 18 behind them (one launch each: the kernel reads one set of tables); in either part the long bands start first
	std::stable_sort(bj, bj + nb, [](const dev::DecBandJob &a, const dev::DecBandJob &b) { return a.table != b.table ? a.table < b.table : a.bytes > b.bytes; });
	const int nb18 = nd, nb17 = nb - nb18;
	memcpy(h_sample_, sample, size);
	HIPCHK(hipMemsetAsync(d_errors_, 0, sizeof(int), st));
	HIPCHK(hipMemcpyAsync(d_sample_, h_sample_, (size + 3) & ~(size_t)3, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(d_bandjobs_, bj, nb * sizeof(dev::DecBandJob), hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(d_lowjobs_, lj, nl * sizeof(dev::DecLowpassJob), hipMemcpyHostToDevice, st));
	(void)hipGetLastError();
	dev::k_dec_bands_par_ll<<<nb17, dev::DECP_LL_THREADS, 0, st>>>((const dev::DecBandJob *)d_bandjobs_, (const dev::DecTables *)d_tables_, d_errors_);
	if (nb18) {
		HIPCHK(hipMemcpyAsync(d_diffjobs_, dj, nd * sizeof(dev::DecDiffJob), hipMemcpyHostToDevice, st));
		dev::k_dec_bands_par_ll<<<nb18, dev::DECP_LL_THREADS, 0, st>>>((const dev::DecBandJob *)d_bandjobs_ + nb17, (const dev::DecTables *)d_tables18_, d_errors_);
		dev::k_dec_undiff<<<dim3((unsigned)nd, dev::DXU_SPLIT), dev::DXU_THREADS, 0, st>>>((const dev::DecDiffJob *)d_diffjobs_, d_errors_, 0);
	}
	dev::k_dec_lowpass<<<dim3(8, (unsigned)nl), 256, 0, st>>>((const dev::DecLowpassJob *)d_lowjobs_);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(h_errors_, d_errors_, sizeof(int), hipMemcpyDeviceToHost, st));
	return 0;
}

int GpuGroupEntropyDecoder::check() { return h_errors_ ? *h_errors_ : -1; }

// =============================================================================================
// GpuGroupBatchEntropyDecoder
// =============================================================================================
void GpuGroupBatchEntropyDecoder::release()
{
	(void)hipSetDevice(device_);
	void *dev[] = { d_tables_, d_tables18_, d_plan_, d_bandjobs_, d_lowjobs_, d_diffjobs_, d_twojobs_, d_errors_ };
	for (void *p : dev) if (p) (void)hipFree(p);
	if (h_errors_) (void)hipHostFree(h_errors_);
	for (void *&e : ev_) if (e) { (void)hipEventDestroy((hipEvent_t)e); e = nullptr; }
	d_tables_ = d_tables18_ = d_plan_ = d_bandjobs_ = d_lowjobs_ = d_diffjobs_ = d_twojobs_ = nullptr; d_errors_ = h_errors_ = nullptr;
	ext_samples_ = ext_followers_ = nullptr; d_verdicts_ = nullptr; active_ = 0; timed_ = false; n_ = 0;
}

int GpuGroupBatchEntropyDecoder::prepare(const GopPlan &plan, int ngroups, int16_t *d_coeffs, size_t stride, int out_kind, void *stream, int device)
{
	int rc = device_init();
	if (rc) return rc;
	release();
	device_ = device >= 0 ? device : device_current(); (void)hipSetDevice(device_);
	plan_ = plan; n_ = ngroups; d_coeffs_ = d_coeffs; coeff_stride_ = stride; out_kind_ = out_kind; stream_ = stream;
	if (n_ < 1 || plan.num_channels != 3) return -1;
	// the device's view of the group pyramid; the coded bands in launch order: by area, largest first (dec_build_plan's rule), code set 17 in front of code set 18
	dev::DecGroupPlan dp;
	memset(&dp, 0, sizeof(dp));
	dp.width = plan.width; dp.height = plan.height; dp.display_height = plan.display_height; dp.interlaced = plan.interlaced ? 1 : 0;
	struct Coded { int c, k, b, table; long long area; };
	std::vector<Coded> coded;
	for (int c = 0; c < 3; c++) {
		dp.low_bias[c] = group_lowpass_bias(plan.ch[c].w[5].width, out_kind, c);
		for (int k = 0; k < kGopWavelets; k++) {
			const GopWavelet &wv = plan.ch[c].w[k];
			for (int b = 0; b < 4; b++) {
				if (wv.offset[b] >= ((size_t)1 << 32)) return -5;
				dp.band[c][k][b] = dev::DecGroupBand{ wv.width, wv.height, wv.pitch, -1, (uint32_t)wv.offset[b] };
				if (k == 2 || b == 0 || b >= wv.nbands) continue;
				// k_dec_bands_par clears its band with 16-byte stores
				if ((wv.offset[b] & 7) || (wv.pitch & 7) || (stride & 7)) return -3;
				const bool diff = gop_band_is_difference_coded(plan, k, b);
				if (diff && wv.width > dev::DXU_MAX * dev::DXU_THREADS) return -3;      // (k_dec_undiff: rows of up to DXU_MAX x DXU_THREADS coefficients)
				coded.push_back(Coded{ c, k, b, diff ? 1 : 0, (long long)wv.pitch * wv.height });
			}
		}
		if (plan.ch[c].w[3].width & 1) return -3;          // (k_dec_lowpass reads a raw band of odd width as unsigned words: the lowpass rule, not w[3]'s)
	}
	// (k_dec_band_two_pass clears subband 7 with 16-byte stores; where it cannot, such a group stays with the host)
	dp.two_pass = 1;
	for (int c = 0; c < 3; c++) if ((plan.ch[c].w[3].offset[0] & 7) || (plan.ch[c].w[3].pitch & 7) || (stride & 7)) dp.two_pass = 0;
	std::stable_sort(coded.begin(), coded.end(), [](const Coded &a, const Coded &b) { return a.table != b.table ? a.table < b.table : a.area > b.area; });
	for (size_t s = 0; s < coded.size(); s++) { dp.band[coded[s].c][coded[s].k][coded[s].b].slot = (int)s; if (coded[s].table) dp.slots18++; else dp.slots17++; }
	slots17_ = dp.slots17; slots18_ = dp.slots18; two_pass_ok_ = dp.two_pass != 0;
	if (slots17_ + slots18_ != kGroupBandJobs || slots18_ != (plan.interlaced ? kGroupDiffJobs : 0)) return -3;
	// one job per workgroup in gridDim.x (k_dec_bands_par, k_dec_undiff), the raw bands in gridDim.y (k_dec_lowpass: 65 535)
	if ((long long)kGroupRawJobs * n_ > 65535) return -5;
	HIPCHK(hipMalloc(&d_plan_, sizeof(dp)));
	HIPCHK(hipMemcpy(d_plan_, &dp, sizeof(dp), hipMemcpyHostToDevice));
	std::vector<uint32_t> t = build_dec_tables(1);
	HIPCHK(hipMalloc(&d_tables_, t.size() * 4));
	HIPCHK(hipMemcpy(d_tables_, t.data(), t.size() * 4, hipMemcpyHostToDevice));
	// (code set 18: the difference-coded bands of interlaced groups, and the two passes of subband 7 of any group from an 8-bit RGB source)
	t = build_dec_tables(2);
	HIPCHK(hipMalloc(&d_tables18_, t.size() * 4));
	HIPCHK(hipMemcpy(d_tables18_, t.data(), t.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMalloc(&d_twojobs_, (size_t)3 * n_ * sizeof(dev::DecTwoPassJob)));
	HIPCHK(hipMalloc(&d_bandjobs_, (size_t)kGroupBandJobs * n_ * sizeof(dev::DecBandJob)));
	HIPCHK(hipMalloc(&d_lowjobs_, (size_t)kGroupRawJobs * n_ * sizeof(dev::DecLowpassJob)));
	HIPCHK(hipMalloc(&d_diffjobs_, (size_t)kGroupDiffJobs * n_ * sizeof(dev::DecDiffJob)));
	HIPCHK(hipMalloc((void **)&d_errors_, sizeof(int)));
	HIPCHK(hipHostMalloc((void **)&h_errors_, sizeof(int), hipHostMallocPortable));
	*h_errors_ = 0;
	for (void *&e : ev_) HIPCHK(hipEventCreate((hipEvent_t *)&e));
	static_assert((int)dev::DEC_GROUP_RAW_JOBS == (int)kGroupRawJobs && (int)dev::DEC_GROUP_DIFF_JOBS == (int)kGroupDiffJobs, "one count of a group's raw and difference jobs");
	return 0;
}

int GpuGroupBatchEntropyDecoder::set_samples_device(const uint8_t *d_samples, const uint32_t *d_sizes, const uint32_t *d_offsets)
{
	// (k_dec_parse_group reads 256-byte windows counted from each sample's start, longword by longword: cfhd_entropy_gpu.hip GpuEntropyDecoder::set_samples_device)
	if (!d_samples || !d_sizes || !d_offsets || ((uintptr_t)d_samples & 255)) return -1;
	ext_samples_ = d_samples; ext_sizes_ = d_sizes; ext_offsets_ = d_offsets; ext_followers_ = nullptr;
	return 0;
}

int GpuGroupBatchEntropyDecoder::set_samples_slots(const uint8_t *d_groups, size_t group_stride, const uint32_t *d_sizes, const uint8_t *d_followers, size_t follower_stride, const uint32_t *d_follower_sizes)
{
	if (!d_groups || !d_sizes || !d_followers || !d_follower_sizes || (((uintptr_t)d_groups | (uintptr_t)d_followers | group_stride | follower_stride) & 255)) return -1;
	ext_samples_ = d_groups; ext_stride_ = group_stride; ext_sizes_ = d_sizes; ext_offsets_ = nullptr;
	ext_followers_ = d_followers; follower_stride_ = follower_stride; ext_follower_sizes_ = d_follower_sizes;
	return 0;
}

const char *GpuGroupBatchEntropyDecoder::band_kernel() const { return par_backend(n_) == DecBackend::ParLowLatency ? "k_dec_bands_par_ll" : "k_dec_bands_par"; }

int GpuGroupBatchEntropyDecoder::launch()
{
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	if (!ext_samples_ || !d_plan_ || (ext_followers_ && !d_verdicts_)) return -1;
	// the groups of this pass: the job tables are [slot][n], the launches n times as long
	const int ng = active_groups();
	const bool slots = ext_followers_ != nullptr;
	// subband 7 coded in two passes: whatever the sample says in the slots of the decode queue; in the coder's dense buffer where the batch's own plan codes it so
	const bool two_pass = slots || (two_pass_ok_ && gop_temporal_lowpass_is_coded(plan_));
	HIPCHK(hipMemsetAsync(d_errors_, 0, sizeof(int), st));
	(void)hipGetLastError();
	// the parser reads the headers and size fields only (k_ent_layout): it runs beside k_ent_emit, the band decoder waits for the payloads
	if (ev_headers_) HIPCHK(hipStreamWaitEvent(st, (hipEvent_t)ev_headers_, 0));
	HIPCHK(hipEventRecord((hipEvent_t)ev_[0], st));
	dev::k_dec_parse_group<<<ng, dev::DEC_PARSE_THREADS, 0, st>>>(ext_samples_, ext_offsets_, ext_sizes_, ng, (const dev::DecGroupPlan *)d_plan_, d_coeffs_, coeff_stride_,
	                                                              (dev::DecBandJob *)d_bandjobs_, (dev::DecLowpassJob *)d_lowjobs_, (dev::DecDiffJob *)d_diffjobs_, d_errors_,
	                                                              ext_stride_, slots ? d_verdicts_ : nullptr, slots ? d_verdicts_ + n_ : nullptr, ext_followers_, follower_stride_, ext_follower_sizes_,
	                                                              two_pass ? (dev::DecTwoPassJob *)d_twojobs_ : nullptr);
	HIPCHK(hipEventRecord((hipEvent_t)ev_[1], st));
	if (ev_payloads_) HIPCHK(hipStreamWaitEvent(st, (hipEvent_t)ev_payloads_, 0));
	ev_headers_ = ev_payloads_ = nullptr;
	HIPCHK(hipEventRecord((hipEvent_t)ev_[2], st));
	// a workgroup per band, the rows of one code set in one launch: few groups in the latency shape (the launch lasts as long as the longest band's serial steps)
	const bool ll = par_backend(ng) == DecBackend::ParLowLatency;
	auto bands = [&](const dev::DecBandJob *jobs, int count, const void *tables) {
		if (ll) dev::k_dec_bands_par_ll<<<count, dev::DECP_LL_THREADS, 0, st>>>(jobs, (const dev::DecTables *)tables, d_errors_);
		else dev::k_dec_bands_par<<<count, dev::DECP_THREADS, 0, st>>>(jobs, (const dev::DecTables *)tables, d_errors_);
	};
	bands((const dev::DecBandJob *)d_bandjobs_, slots17_ * ng, d_tables_);
	if (slots18_) {
		bands((const dev::DecBandJob *)d_bandjobs_ + (size_t)slots17_ * ng, slots18_ * ng, d_tables18_);
		dev::k_dec_undiff<<<dim3((unsigned)(kGroupDiffJobs * ng), dev::DXU_SPLIT), dev::DXU_THREADS, 0, st>>>((const dev::DecDiffJob *)d_diffjobs_, d_errors_, 0);
	}
	if (two_pass) {
		// subband 7 of the groups from 8-bit RGB sources: a workgroup per (group, channel), the jobs of raw-word groups are empty
		HIPCHK(hipEventRecord((hipEvent_t)ev_[5], st));
		dev::k_dec_band_two_pass<<<3 * ng, dev::DECP_THREADS, 0, st>>>((const dev::DecTwoPassJob *)d_twojobs_, (const dev::DecTables *)d_tables18_, d_errors_);
	}
	two_pass_timed_ = two_pass;
	HIPCHK(hipEventRecord((hipEvent_t)ev_[3], st));
	dev::k_dec_lowpass<<<dim3(8, (unsigned)(kGroupRawJobs * ng)), 256, 0, st>>>((const dev::DecLowpassJob *)d_lowjobs_);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord((hipEvent_t)ev_[4], st));
	timed_ = true;
	HIPCHK(hipMemcpyAsync(h_errors_, d_errors_, sizeof(int), hipMemcpyDeviceToHost, st));
	return 0;
}

int GpuGroupBatchEntropyDecoder::check() { return h_errors_ ? (*h_errors_ ? -1 : 0) : -1; }

float GpuGroupBatchEntropyDecoder::kernel_ms(int k)
{
	float ms = 0;
	if (!timed_ || k < 0 || k > 3 || (k == 3 && !two_pass_timed_)) return 0;
	void *a = k == 0 ? ev_[0] : (k == 1 ? ev_[2] : (k == 2 ? ev_[3] : ev_[5])), *b = k == 0 ? ev_[1] : (k == 2 ? ev_[4] : ev_[3]);
	if (hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return ms;
}

// ---- k_dec_parse by itself (cfhd_entropy_gpu.h DecParseTables)
int dec_parse_tables_prepare(const FramePlan &plan, int n, DecParseTables *t)
{
	dec_parse_tables_release(t);
	if (n < 1) return -1;
	dev::DecPlan dp;
	dec_build_plan(plan, plan.pixel_kind, &dp);
	t->n = n; t->nch = plan.num_channels;
	const size_t lows = (size_t)n * plan.num_channels;
	HIPCHK(hipMalloc(&t->d_plan, sizeof(dp)));
	HIPCHK(hipMemcpy(t->d_plan, &dp, sizeof(dp), hipMemcpyHostToDevice));
	HIPCHK(hipMalloc(&t->d_bandjobs, lows * 9 * sizeof(dev::DecBandJob)));
	HIPCHK(hipMalloc(&t->d_lowjobs, lows * sizeof(dev::DecLowpassJob)));
	HIPCHK(hipMalloc(&t->d_diffjobs, lows * sizeof(dev::DecDiffJob)));
	HIPCHK(hipMalloc((void **)&t->d_errors, sizeof(int)));
	HIPCHK(hipMemset(t->d_lowjobs, 0, lows * sizeof(dev::DecLowpassJob)));
	HIPCHK(hipMemset(t->d_errors, 0, sizeof(int)));
	return 0;
}

void dec_parse_tables_release(DecParseTables *t)
{
	void *dv[] = { t->d_plan, t->d_bandjobs, t->d_lowjobs, t->d_diffjobs, t->d_errors };
	for (void *p : dv) if (p) (void)hipFree(p);
	*t = DecParseTables();
}

int dec_parse_launch(const DecParseTables &t, const uint8_t *d_slots, size_t slot_stride, const uint32_t *d_sizes, int count, uint32_t *d_verdicts, void *stream)
{
	if (!t.d_plan || !d_slots || !d_sizes || !d_verdicts || count < 1 || count > t.n || ((uintptr_t)d_slots & 255) || (slot_stride & 255)) return -1;
	dev::k_dec_parse<<<count, dev::DEC_PARSE_THREADS, 0, (hipStream_t)stream>>>(d_slots, slot_stride, d_sizes, count, (const dev::DecPlan *)t.d_plan, nullptr, 0,
		(dev::DecBandJob *)t.d_bandjobs, (dev::DecLowpassJob *)t.d_lowjobs, t.d_errors, (dev::DecDiffJob *)t.d_diffjobs, nullptr, d_verdicts);
	HIPCHK(hipGetLastError());
	return 0;
}

} // namespace cfhd
