// cfhd_device.hip -- HIP runtime glue: device selection, HBM/pinned buffers, job tables and kernel launches.
//
// Replaces the reference's per-encoder scratch + thread pool (EncoderSDK/AsyncEncoder.cpp, Codec/thread.c) with
// HIP streams: a batch owns one stream; H2D copy, the three forward (or inverse) launches and the D2H copy are
// queued back to back on it, batches on different streams overlap.
#include "cfhd_device.h"
#include "cfhd_kernels.h"
#include "cfhd_collect_kernels.h"
#include <hip/hip_runtime.h>
#include <string.h>
#include <stddef.h>
#include <vector>
#include <stdlib.h>
#include <stdio.h>
#include <mutex>
#include <thread>
#include <atomic>
#include <string>
#include <utility>

namespace cfhd {

namespace {
// Text of the last failure: written from whatever thread failed (the chunks of a batch run on threads of their own), read through cfhd_amd_last_error()
std::string g_err_text; std::mutex g_err_mutex;
thread_local std::string t_err_copy;
struct ErrSlot { ErrSlot &operator=(const char *t) { std::lock_guard<std::mutex> l(g_err_mutex); g_err_text = t; return *this; } } g_err;
std::once_flag g_init_once;
int g_init_rc = -1;
int g_device = 0;

int fail(hipError_t e, const char *what)
{
	char buf[256];
	snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
	g_err = buf;
	return (int)e ? (int)e : -1;
}
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(_e, #expr); } while (0)

dev::QuantParam make_q(int divisor, int mpq)
{
	dev::QuantParam q; q.divisor = divisor; q.mid = 0; q.mult = 0;
	if (divisor > 1) {
		if (mpq >= 2 && mpq < 9) { q.mid = divisor / mpq; if (mpq == 2 && q.mid) q.mid--; }   // quantize.c:1415-1427
		q.mult = ((1u << 16) / (unsigned)divisor) & 0xffffu;
	}
	return q;
}

struct EncJobs {            // layout of the job table buffer of an EncodeBatch
	dev::FwdYuvJob *yuv;    // [n]         level 1 of the packed 4:2:2 formats
	dev::FwdPlaneJob *l2;   // [n * nch]
	dev::FwdPlaneJob *l3;   // [n * nch]
	dev::FwdPlaneJob *l1;   // [n * nch]   level 1 of the interleaved 16-bit 4:4:4(:4) formats (k_fwd_packed16) and of the Bayer planes (k_fwd_plane)
	dev::BayerJob *bayer;   // [n]         Bayer mosaic -> component planes (k_unpack_byr4)
};
EncJobs enc_jobs_at(void *base, int n, int nch)
{
	EncJobs j;
	j.yuv = (dev::FwdYuvJob *)base;
	j.l2 = (dev::FwdPlaneJob *)(j.yuv + n);
	j.l3 = j.l2 + (size_t)n * nch;
	j.l1 = j.l3 + (size_t)n * nch;
	j.bayer = (dev::BayerJob *)(j.l1 + (size_t)n * nch);
	return j;
}
size_t enc_jobs_bytes(int n, int nch) { return (size_t)n * sizeof(dev::FwdYuvJob) + 3 * (size_t)n * nch * sizeof(dev::FwdPlaneJob) + (size_t)n * sizeof(dev::BayerJob); }

struct DecJobs { dev::InvPlaneJob *l3, *l2; dev::InvYuvJob *yuv; dev::InvPlaneJob *l1; /* last level of the 4:4:4(:4) formats (k_inv_packed16) */ dev::HalfYuvJob *half; /* [n] half-resolution output */ dev::HalfPackedJob *halfp; /* [n] the same for the 4:4:4(:4) formats */ dev::InvBayerJob *bayer; /* [n] BYR4 output: the mosaic and the restore table (k_inv_bayer_strip, beside l1) */ };
DecJobs dec_jobs_at(void *base, int n, int nch)
{
	DecJobs j;
	j.l3 = (dev::InvPlaneJob *)base;
	j.l2 = j.l3 + (size_t)n * nch;
	j.yuv = (dev::InvYuvJob *)(j.l2 + (size_t)n * nch);
	j.l1 = (dev::InvPlaneJob *)(j.yuv + n);
	j.half = (dev::HalfYuvJob *)(j.l1 + (size_t)n * nch);
	j.halfp = (dev::HalfPackedJob *)(j.half + n);
	j.bayer = (dev::InvBayerJob *)(j.halfp + n);
	return j;
}
size_t dec_jobs_bytes(int n, int nch) { return 3 * (size_t)n * nch * sizeof(dev::InvPlaneJob) + (size_t)n * sizeof(dev::InvYuvJob) + (size_t)n * sizeof(dev::HalfYuvJob) + (size_t)n * sizeof(dev::HalfPackedJob) + (size_t)n * sizeof(dev::InvBayerJob); }

// Word of component plane c inside an interleaved 16-bit pixel: planes are G, R, B(, A) (frame.c:6128-6157, convert.c:6750-6752),
// RG48 pixels are R, G, B; b64a pixels are A, R, G, B (frame.c:6676-6683).
int packed_word_of_channel(int pixel_kind, int c)
{
	static const int rg48[4] = { 1, 0, 2, 3 }, b64a[4] = { 2, 1, 3, 0 };
	return (pixel_kind == PIX_B64A ? b64a : rg48)[c & 3];
}
bool is_packed16(int pixel_kind) { return pixel_kind == PIX_RG48 || pixel_kind == PIX_B64A; }
// decoder outputs made of 16-bit words that k_inv_packed16 writes plane by plane: the interleaved RGB(A) pixels, and YU64 (words Y0 C1 Y1 C2:
// luma every second word, the half-width chroma planes every fourth; the reference decodes 4:2:2 samples to YU64 through the same planar
// 16-bit rows as RGB 4:4:4 to RG48, oracle/cfhd_oracle_inv.c orc_inv_spatial_to_yu64)
// ... and the 8-bit RGB pixels B, G, R(, A) of RGB 4:4:4 samples (RG24, BGRA: bottom row first; BGRa: top row first), which the same kernel writes
// in its byte mode: the 12-bit component doubled + 9 + a four-bit dither, >> 5 (orc_inv_spatial_to_rgb8: the reference's model)
static bool dec_rgb8(int out_kind) { return out_kind == PIX_RG24 || out_kind == PIX_BGRA || out_kind == PIX_BGRa; }
static int rgb8_bytes(int out_kind) { return out_kind == PIX_RG24 ? 3 : 4; }
// ... and the 10-bit RGB words (r210, DPX0: big-endian; AB10, AR10: little-endian) through k_inv_rgb10 (orc_inv_spatial_to_rgb10)
static bool dec_rgb10(int out_kind) { return out_kind >= PIX_R210 && out_kind <= PIX_AR10; }
// planes of the sample that reach the output pixel: an RGBA 4:4:4:4 sample decoded to RG48 leaves its alpha plane behind (the reference's RG48 route on planes G, R, B;
// pinned on eight geometries, tests/test_oracle_vs_ref.py)
static int dec_out_channels(int out_kind, const FramePlan &plan) { return out_kind == PIX_RG48 && plan.encoded_format == ENC_RGBA4444 ? 3 : plan.num_channels; }
// position of plane c inside the pixel: 16-bit word, or byte for the 8-bit formats (planes G, R, B(, A) -> bytes 1, 2, 0(, 3))
static int dec_word_of_channel(int out_kind, int c) { return dec_rgb10(out_kind) ? 0 : out_kind == PIX_YU64 ? (c == 0 ? 0 : (c == 1 ? 1 : 3)) : (dec_rgb8(out_kind) ? (c == 0 ? 1 : (c == 1 ? 2 : (c == 2 ? 0 : 3))) : packed_word_of_channel(out_kind, c)); }
static int dec_stride_of_channel(int out_kind, int c, int nch) { return out_kind == PIX_YU64 ? (c == 0 ? 2 : 4) : (dec_rgb8(out_kind) ? rgb8_bytes(out_kind) : (dec_rgb10(out_kind) ? 3 : (out_kind == PIX_B64A ? 4 : nch))); }     // (b64a from RGB 4:4:4: three planes, four words)
static int dec_words_per_position(int out_kind, int nch) { return out_kind == PIX_YU64 ? 2 : (dec_rgb8(out_kind) ? rgb8_bytes(out_kind) : (out_kind == PIX_B64A ? 4 : nch)); }
static int16_t *dec_plane_out(void *frame, int out_kind, int c) { return dec_rgb8(out_kind) ? (int16_t *)((uint8_t *)frame + dec_word_of_channel(out_kind, c)) : (int16_t *)((uint16_t *)frame + dec_word_of_channel(out_kind, c)); }
// encoder input made of 16-bit words that k_fwd_packed16 picks apart (per channel: first word, words from sample to sample, right shift).
// YU64 (Codec/frame.c:1556 ConvertYU64ToFrame16s + convert.c:3345, :14375): words Y0 C1 Y1 C2, every word >> 6 to 10 bits, channel 1 = C1, 2 = C2.
// v210 (frame.c:1431 ConvertV210ToFrame16s): three 10-bit samples per 32-bit word, FwdPlaneJob::layout tells the loader which component to pick.
// RG24 (frame.c:6173 ConvertRGBtoRGB48): bytes B, G, R, bottom row first, byte << 4; planes G, R, B.
// The Avid 4:2:2 layouts (frame.c:13144-13515): Cb Y1 Cr Y2 per pixel pair as bytes (avu8), 16-bit words (av16, a106: the same arithmetic), signed 2.14 words (a214)
// or -- av28 -- a plane of two-bit fields and a plane of bytes; FwdPlaneJob::layout names the arithmetic (avid_layout).
static bool enc_packed16(int pixel_kind) { return is_packed16(pixel_kind) || pixel_kind == PIX_RG64 || pixel_kind == PIX_YU64 || pixel_kind == PIX_V210 || pixel_kind == PIX_RG24 || pixel_kind == PIX_BGRA || pixel_kind == PIX_BGRa || (pixel_kind >= PIX_R210 && pixel_kind <= PIX_AR10) || is_avid_422(pixel_kind); }
static int avid_layout(int pixel_kind) { return pixel_kind == PIX_AVU8 ? dev::FWD_AVID_BYTES8 : (pixel_kind == PIX_A214 ? dev::FWD_AVID_S214 : (pixel_kind == PIX_AV28 ? dev::FWD_AVID_2_8 : dev::FWD_AVID_WORDS16)); }
// av28: the reference finds the lower plane width x height / 2 bytes into the frame, with the ENCODED height (frame.c:13180 takes the plane's, a multiple of 8), and
// walks both planes as tightly packed rows whatever the pitch (:13185-13186).  The frame as it is copied: the upper plane up to there, display_height rows of the lower.
static size_t av28_lower_plane_offset(int width, int height) { return (size_t)width * height / 2; }
static size_t av28_frame_bytes(int width, int height, int display_height) { return av28_lower_plane_offset(width, height) + (size_t)width * 2 * display_height; }
static bool enc_bytes8(int pixel_kind) { return pixel_kind == PIX_RG24 || pixel_kind == PIX_BGRA || pixel_kind == PIX_BGRa; }
static bool enc_rgb10(int pixel_kind) { return pixel_kind >= PIX_R210 && pixel_kind <= PIX_AR10; }
// bit position of plane c (G, R, B) inside the pixel word of the 10-bit RGB formats
static int rgb10_shift(int pixel_kind, int c) { const int r = pixel_kind == PIX_DPX0 ? 22 : (pixel_kind == PIX_AB10 ? 0 : 20), g = pixel_kind == PIX_DPX0 ? 12 : 10, b = pixel_kind == PIX_DPX0 ? 2 : (pixel_kind == PIX_AB10 ? 20 : 0); return c == 0 ? g : (c == 1 ? r : b); }
// RG48 / b64a encoded as YUV 4:2:2: the loader of k_fwd_packed16 converts the pixels (FWD_RGB16_AS_422); every plane reads from the R word
static bool enc_rgb_as_422(const FramePlan &plan) { return (is_packed16(plan.pixel_kind) || plan.pixel_kind == PIX_RG64) && plan.encoded_format == ENC_YUV422; }
static int enc_word_of_channel(int pixel_kind, int c) { return pixel_kind == PIX_V210 || enc_bytes8(pixel_kind) || enc_rgb10(pixel_kind) ? 0 : (pixel_kind == PIX_YU64 ? (c == 0 ? 0 : (c == 1 ? 1 : 3)) : packed_word_of_channel(pixel_kind, c)); }
static int enc_stride_of_channel(int pixel_kind, int c, int nch) { return pixel_kind == PIX_YU64 ? (c == 0 ? 2 : 4) : (pixel_kind == PIX_B64A || pixel_kind == PIX_RG64 ? 4 : nch); }     // (b64a / RG64 to RGB 4:4:4 have three planes of four-word pixels)
// The loader of k_fwd_packed16 / k_fwd_gop_packed16 for plane c of one packed frame (FwdPlaneJob: in, in_pitch, xstride, shift, display_height, compand, layout,
// tail_from), written in one place for the intra batches and the two-frame groups: it reads the frame where fill_fwd_plane_job's job reads a plane.
static void fill_packed16_loader(dev::FwdPlaneJob &p, const uint8_t *frame8, int in_pitch, int pixel_kind, int encoded_format, int color_matrix, int width, int height, int precision,
                                 int display_height, int nch, int c)
{
	if (is_avid_422(pixel_kind)) {           // planes Y, Cr, Cb of samples Cb Y1 Cr Y2
		p.in = (const int16_t *)frame8; p.in_pitch = pixel_kind == PIX_AV28 ? 2 * width : in_pitch; p.display_height = display_height; p.compand = 0;
		p.layout = avid_layout(pixel_kind); p.tail_from = c == 0 ? 1 : (c == 1 ? 2 : 0); p.xstride = c == 0 ? 2 : 4;
		p.shift = pixel_kind == PIX_AV28 ? (int)av28_lower_plane_offset(width, height) : 0;
		return;
	}
	const uint16_t *frame = (const uint16_t *)frame8;
	p.in = (const int16_t *)(frame + enc_word_of_channel(pixel_kind, c)); p.in_pitch = in_pitch / 2;
	p.xstride = enc_stride_of_channel(pixel_kind, c, nch); p.shift = 16 - precision; p.display_height = display_height;
	p.compand = (pixel_kind == PIX_B64A || pixel_kind == PIX_RG64) && c == 3;
	p.layout = pixel_kind == PIX_V210 ? dev::FWD_V210_Y + c : dev::FWD_WORDS16; p.tail_from = (width - width % 48) / 2;
	if (enc_bytes8(pixel_kind)) { p.layout = pixel_kind == PIX_BGRa ? dev::FWD_BYTES8_TOP_DOWN : dev::FWD_BYTES8_BOTTOM_UP; p.in_pitch = in_pitch; p.xstride = pixel_kind == PIX_RG24 ? 3 : 4; p.tail_from = c == 0 ? 1 : (c == 1 ? 2 : (c == 2 ? 0 : 3)); p.compand = c == 3; }     // planes G, R, B(, A) of bytes B, G, R(, A)
	if (enc_rgb10(pixel_kind)) { p.layout = dev::FWD_RGB10; p.in_pitch = in_pitch / 4; p.xstride = pixel_kind == PIX_R210 || pixel_kind == PIX_DPX0; p.tail_from = rgb10_shift(pixel_kind, c); }
	if ((is_packed16(pixel_kind) || pixel_kind == PIX_RG64) && encoded_format == ENC_YUV422) {      // (enc_rgb_as_422)
		p.in = (const int16_t *)(frame + (pixel_kind == PIX_B64A ? 1 : 0));
		p.layout = dev::FWD_RGB16_AS_422; p.xstride = pixel_kind == PIX_RG48 ? 3 : 4; p.tail_from = c; p.shift = color_matrix; p.compand = 0;
	}
	if (enc_bytes8(pixel_kind) && encoded_format == ENC_YUV422) { p.layout = pixel_kind == PIX_BGRa ? dev::FWD_BYTES8_AS_422_TOP_DOWN : dev::FWD_BYTES8_AS_422_BOTTOM_UP; p.tail_from = c; p.shift = color_matrix; }
}

// The level-1 wavelet of one frame as its first (encoder) or last (decoder) launch sees it: a frame of an intra batch, or frame f of a two-frame group (w[f]: what the
// temporal step reads, what the temporal inverse leaves).  The plan types stop here: the job fillers below read this.
struct Level1 { int16_t *band[kMaxChannels][4]; int pitch[kMaxChannels], width[kMaxChannels], height[kMaxChannels], quant[kMaxChannels][4]; };
Level1 level1_of(const FramePlan &plan, int16_t *base)
{
	Level1 l;
	for (int c = 0; c < plan.num_channels; c++) { const BandDesc *b = plan.ch[c].band[0]; l.pitch[c] = b[0].pitch; l.width[c] = b[0].width; l.height[c] = b[0].height; for (int k = 0; k < 4; k++) { l.band[c][k] = base + b[k].offset; l.quant[c][k] = b[k].quant; } }
	return l;
}
Level1 level1_of(const GopPlan &plan, int f, int16_t *base)
{
	Level1 l;
	for (int c = 0; c < 3; c++) { const GopWavelet &w = plan.ch[c].w[f]; l.pitch[c] = w.pitch; l.width[c] = w.width; l.height[c] = w.height; for (int k = 0; k < 4; k++) { l.band[c][k] = base + w.offset[k]; l.quant[c][k] = w.quant[k]; } }
	return l;
}
// The four bands a forward job writes, with their divisors: channel c of a level-1 wavelet, a wavelet of an intra pyramid, a wavelet of a group
struct FwdBands { int16_t *out[4]; int pitch, quant[4]; };
FwdBands fwd_bands(const Level1 &l, int c) { FwdBands d; d.pitch = l.pitch[c]; for (int b = 0; b < 4; b++) { d.out[b] = l.band[c][b]; d.quant[b] = l.quant[c][b]; } return d; }
FwdBands fwd_bands(int16_t *base, const BandDesc *w) { FwdBands d; d.pitch = w[0].pitch; for (int b = 0; b < 4; b++) { d.out[b] = base + w[b].offset; d.quant[b] = w[b].quant; } return d; }
FwdBands fwd_bands(int16_t *base, const GopWavelet &w) { FwdBands d; d.pitch = w.pitch; for (int b = 0; b < 4; b++) { d.out[b] = base + w.offset[b]; d.quant[b] = w.quant[b]; } return d; }

// One job of each forward family, for the intra batches and the two-frame groups alike.  Level 1 of a packed 8-bit 4:2:2 frame (k_fwd_yuv422 and its strip forms;
// interlaced: k_fwd_frame_yuv422, the same table read as FwdFrameJob); FwdYuvJob::lists is EncodeBatch::fill_block_lists's.
void fill_fwd_yuv_job(dev::FwdYuvJob &y, const uint8_t *in, int in_pitch, int width, int height, int display_height, int pixel_kind, int precision, const Level1 &l, int mpq, bool interlaced)
{
	y.in = in; y.in_pitch = in_pitch;
	y.width = width; y.height = height; y.display_height = display_height;
	y.uyvy = pixel_kind == PIX_2VUY; y.shift = precision - 8;
	for (int c = 0; c < 3; c++) {
		y.out_pitch[c] = l.pitch[c];
		for (int b = 0; b < 4; b++) { y.out[c][b] = l.band[c][b]; y.q[c][b] = make_q(l.quant[c][b], mpq); }
		// interlaced: the difference-coded band is quantized inside the horizontal filter, midpoint = divisor / prequant without the decrement (spatial.c:5360-5363)
		const int dq = l.quant[c][2];
		if (interlaced && dq > 1 && mpq >= 2 && mpq < 9) y.q[c][2].mid = dq / mpq;
	}
}
// One wavelet of a plane of 16-bit samples (k_fwd_plane, k_fwd_plane_strip): levels 2 and 3, the Bayer component planes, the group's spatial wavelets.  Sets every field a
// kernel reads; a job of the packed-16 loaders passes no plane and lets fill_packed16_loader say how the frame is read instead.
void fill_fwd_plane_job(dev::FwdPlaneJob &p, const int16_t *in, int in_pitch, int width, int height, int prescale, const FwdBands &d, int mpq)
{
	p.in = in; p.in_pitch = in_pitch; p.width = width; p.height = height; p.prescale = prescale;
	p.xstride = 1; p.shift = 0; p.display_height = height; p.compand = 0; p.layout = dev::FWD_WORDS16; p.tail_from = 0; p.curve = nullptr;
	p.out_pitch = d.pitch;
	for (int b = 0; b < 4; b++) { p.out[b] = d.out[b]; p.q[b] = make_q(d.quant[b], mpq); }
}
} // namespace

const char *device_last_error() { std::lock_guard<std::mutex> l(g_err_mutex); t_err_copy = g_err_text; return t_err_copy.c_str(); }
void device_set_last_error(const char *text) { g_err = text; }

namespace {
std::mutex g_pins_mutex;
std::vector<std::pair<uintptr_t, size_t>> g_pins;
}
int host_buffer_register(void *p, size_t bytes)
{
	if (!p || !bytes) return -1;
	int rc = device_init();
	if (rc) return rc;
	std::lock_guard<std::mutex> lk(g_pins_mutex);
	for (auto &e : g_pins) if (e.first == (uintptr_t)p) return e.second >= bytes ? 0 : -1;
	HIPCHK(hipHostRegister(p, bytes, hipHostRegisterPortable));
	g_pins.push_back({ (uintptr_t)p, bytes });
	return 0;
}
int host_buffer_unregister(void *p)
{
	std::lock_guard<std::mutex> lk(g_pins_mutex);
	for (size_t i = 0; i < g_pins.size(); i++) if (g_pins[i].first == (uintptr_t)p) {
		g_pins.erase(g_pins.begin() + (ptrdiff_t)i);
		HIPCHK(hipHostUnregister(p));
		return 0;
	}
	return -1;
}
bool host_buffer_is_registered(const void *p, size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_pins_mutex);
	for (auto &e : g_pins) if ((uintptr_t)p >= e.first && (uintptr_t)p + bytes <= e.first + e.second) return true;
	return false;
}

// ---- streams (cfhd_device.h)
static thread_local bool t_scope = false;
static thread_local void *t_scope_stream = nullptr;
static std::mutex g_shared_mutex;
static std::vector<void *> g_shared_streams;
int device_stream_create(void **stream)
{
	if (t_scope && t_scope_stream) { *stream = t_scope_stream; return 0; }
	hipStream_t s;
	const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
	if (e != hipSuccess) return (int)e;
	*stream = (void *)s;
	if (t_scope) { t_scope_stream = (void *)s; std::lock_guard<std::mutex> lk(g_shared_mutex); g_shared_streams.push_back((void *)s); }
	return 0;
}
void device_stream_destroy(void *stream)
{
	if (!stream) return;
	{ std::lock_guard<std::mutex> lk(g_shared_mutex); for (void *p : g_shared_streams) if (p == stream) return; }      // a scope's stream: its owner releases it
	(void)hipStreamDestroy((hipStream_t)stream);
}
void device_stream_release(void *stream)
{
	if (!stream) return;
	{ std::lock_guard<std::mutex> lk(g_shared_mutex); for (size_t i = 0; i < g_shared_streams.size(); i++) if (g_shared_streams[i] == stream) { g_shared_streams.erase(g_shared_streams.begin() + (long)i); break; } }
	(void)hipStreamDestroy((hipStream_t)stream);
}
static thread_local bool t_lean = false;
void device_streams_lean(bool on) { t_lean = on; }
bool device_streams_are_lean() { return t_lean; }
StreamScope::StreamScope() { t_scope = true; t_scope_stream = nullptr; }
StreamScope::StreamScope(void *preset) { t_scope = true; t_scope_stream = preset; }
StreamScope::~StreamScope() { t_scope = false; t_scope_stream = nullptr; }
void *StreamScope::stream() const { return t_scope_stream; }

int device_count()
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// The device the calling thread prepares its objects on: the process default (CFHD_AMD_DEVICE / LOCAL_RANK / 0) unless the thread asked for
// another one -- a worker of an encoder pool that spreads over the node's GPUs, a decoder handle that was dealt one (cfhd_api.cpp).
static thread_local int t_device = -1;
int device_select(int dev)
{
	t_device = dev;
	const int rc = device_init();
	return rc ? -1 : device_current();
}
int device_current() { return t_device >= 0 ? t_device : g_device; }

namespace {
struct StageOrder { std::mutex m; hipEvent_t ev[2] = { nullptr, nullptr }; bool recorded[2] = { false, false }; std::atomic<int> passes{0}; /* device_pass_begin / _end */ };
StageOrder *stage_order_of(int device)
{
	static std::mutex m; static std::vector<StageOrder *> all;       // (never freed: events of a device live as long as the process)
	std::lock_guard<std::mutex> lk(m);
	if (device < 0) return nullptr;
	if ((size_t)device >= all.size()) all.resize((size_t)device + 1, nullptr);
	if (!all[device]) all[device] = new StageOrder;
	return all[device];
}
}
int stage_order_wait(int device, int stage, void *stream)
{
	StageOrder *o = stage_order_of(device);
	if (!o || stage < 0 || stage > 1) return -1;
	std::lock_guard<std::mutex> lk(o->m);
	if (o->recorded[stage]) HIPCHK(hipStreamWaitEvent((hipStream_t)stream, o->ev[stage], 0));
	return 0;
}
int stage_order_done(int device, int stage, void *stream)
{
	StageOrder *o = stage_order_of(device);
	if (!o || stage < 0 || stage > 1) return -1;
	std::lock_guard<std::mutex> lk(o->m);
	(void)hipSetDevice(device);
	if (!o->ev[stage]) HIPCHK(hipEventCreateWithFlags(&o->ev[stage], hipEventDisableTiming));
	HIPCHK(hipEventRecord(o->ev[stage], (hipStream_t)stream));
	o->recorded[stage] = true;
	return 0;
}
// Passes in flight (cfhd_device.h): one counter per device, beside the device's stage order.
void device_pass_begin(int device) { if (StageOrder *o = stage_order_of(device)) o->passes.fetch_add(1); }
void device_pass_end(int device) { if (StageOrder *o = stage_order_of(device)) o->passes.fetch_sub(1); }
int device_passes_in_flight(int device) { StageOrder *o = stage_order_of(device); return o ? o->passes.load() : 0; }
int device_caller_save() { int d = -1; if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); return -1; } return d; }
void device_caller_restore(int dev) { if (dev >= 0) { int now = -1; if (hipGetDevice(&now) == hipSuccess && now != dev) (void)hipSetDevice(dev); } }

int device_init()
{
	std::call_once(g_init_once, [] {
		int n = 0;
		hipError_t e = hipGetDeviceCount(&n);
		if (e != hipSuccess || n <= 0) { g_err = "no HIP device available (libcfhd_amd has no CPU fallback)"; g_init_rc = e ? (int)e : -1; return; }
		const char *env = getenv("CFHD_AMD_DEVICE");
		if (!env) env = getenv("LOCAL_RANK");
		g_device = env ? atoi(env) % n : 0;
		e = hipSetDevice(g_device);
		if (e != hipSuccess) { fail(e, "hipSetDevice"); g_init_rc = (int)e; return; }
		g_init_rc = 0;
	});
	if (g_init_rc == 0) {
		int n = 1; (void)hipGetDeviceCount(&n);
		if (t_device >= n) t_device = t_device % (n > 0 ? n : 1);
		hipSetDevice(device_current());              // per calling thread
	}
	return g_init_rc;
}

int packed_frame_pitch(int pixel_kind, int width)
{
	switch (pixel_kind) {
	case PIX_YUY2: case PIX_2VUY: return width * 2;
	case PIX_RG48: return width * 6;
	case PIX_B64A: case PIX_RG64: return width * 8;
	case PIX_BYR4: return width * 2;
	case PIX_BYR5: return width * 3;       // per row PAIR of the mosaic: 4 x width / 2 samples of 12 bits (the unit the frame is laid out in)
	case PIX_YU64: case PIX_AV16: case PIX_A214: case PIX_A106: return width * 4;
	case PIX_AVU8: return width * 2;
	case PIX_AV28: return 0;               // two planes of different row sizes: one block of av28_frame_bytes (EncodeBatch::prepare, GopBatch::prepare)
	case PIX_RG24: return width * 3;
	case PIX_BGRA: case PIX_BGRa: case PIX_R210: case PIX_DPX0: case PIX_AB10: case PIX_AR10: return width * 4;
	case PIX_V210: return (width + 47) / 48 * 128;      // six pixels in 16 bytes, rows padded to 48 pixels (Example/utils.cpp:84-90)
	default: return 0;
	}
}

// =============================================================================================
// EncodeBatch
// =============================================================================================
EncodeBatch::EncodeBatch() {}
EncodeBatch::~EncodeBatch() { release(); }

void EncodeBatch::release()
{
	(void)hipSetDevice(device_);
	if (stream_) hipStreamSynchronize((hipStream_t)stream_);
	ent_ready_ = false;
	if (d_in_) hipFree(d_in_);
	if (h_in_) hipHostFree(h_in_);
	if (d_coeff_) hipFree(d_coeff_);
	if (h_coeff_) hipHostFree(h_coeff_);
	if (d_jobs_) hipFree(d_jobs_);
	if (h_jobs_) hipHostFree(h_jobs_);
	if (d_planes_) hipFree(d_planes_);
	if (d_curve_) hipFree(d_curve_);
	d_planes_ = nullptr; d_curve_ = nullptr;
	if (ev0_) hipEventDestroy((hipEvent_t)ev0_);
	if (ev1_) hipEventDestroy((hipEvent_t)ev1_);
	for (int k = 0; k < 2; k++) if (evl_[k]) { hipEventDestroy((hipEvent_t)evl_[k]); evl_[k] = nullptr; }
	collect_.release();
	if (stream_) device_stream_destroy(stream_);
	d_in_ = h_in_ = nullptr; d_coeff_ = h_coeff_ = nullptr; d_jobs_ = h_jobs_ = nullptr; stream_ = ev0_ = ev1_ = nullptr; n_ = 0;
}

int EncodeBatch::prepare(const FramePlan &plan, int nframes)
{
	int rc = device_init();
	if (rc) return rc;
	release();
	device_ = device_current(); (void)hipSetDevice(device_);      // (release() went to the device of the buffers it freed)
	const bool bayer = plan.pixel_kind == PIX_BYR4 || plan.pixel_kind == PIX_BYR5;
	if (plan.pixel_kind != PIX_YUY2 && plan.pixel_kind != PIX_2VUY && !enc_packed16(plan.pixel_kind) && !bayer) { g_err = "pixel format not supported by the GPU path yet"; return -2; }
	plan_ = plan; n_ = nframes; frame_plans_.clear();
	HIPCHK((hipError_t)device_stream_create(&stream_));
	HIPCHK(hipEventCreate((hipEvent_t *)&ev0_));
	HIPCHK(hipEventCreate((hipEvent_t *)&ev1_));
	for (int k = 0; k < 2; k++) HIPCHK(hipEventCreate((hipEvent_t *)&evl_[k]));
	// Bayer: the plan describes the component planes (half the mosaic in both directions)
	in_pitch_ = packed_frame_pitch(plan.pixel_kind, bayer ? 2 * plan.width : plan.width);
	in_rows_ = plan.pixel_kind == PIX_BYR4 ? 2 * plan.display_height : plan.display_height;      // (BYR5: one packed row per row pair)
	if (plan.pixel_kind == PIX_AV28) { in_pitch_ = (int)av28_frame_bytes(plan.width, plan.height, plan.display_height); in_rows_ = 1; }      // the whole frame as one row
	frame_bytes_ = (size_t)in_pitch_ * in_rows_;
	if (bayer) {
		plane_elems_ = (size_t)plan.ch[0].band[0][0].pitch * 2 * plan.height;           // plane pitch = 2 x the level-1 band pitch (multiple of 16)
		HIPCHK(hipMalloc((void **)&d_planes_, plane_elems_ * 2 * 4 * n_));
		std::vector<uint16_t> curve((size_t)1 << kBayerCurveBits);
		build_bayer_log90_curve(plan.precision, curve.data());
		HIPCHK(hipMalloc((void **)&d_curve_, curve.size() * 2));
		HIPCHK(hipMemcpy(d_curve_, curve.data(), curve.size() * 2, hipMemcpyHostToDevice));
	}
	HIPCHK(hipMalloc((void **)&d_in_, frame_bytes_ * n_));
	HIPCHK(hipHostMalloc((void **)&h_in_, frame_bytes_ * n_, hipHostMallocPortable));
	HIPCHK(hipMalloc((void **)&d_coeff_, (size_t)plan.coeff_elems * 2 * n_));
	HIPCHK(hipMemsetAsync(d_coeff_, 0, (size_t)plan.coeff_elems * 2 * n_, (hipStream_t)stream_));   // pad columns stay zero forever
	HIPCHK(hipHostMalloc((void **)&h_coeff_, (size_t)plan.final_elems * 2 * n_, hipHostMallocPortable));
	jobs_bytes_ = enc_jobs_bytes(n_, plan.num_channels);
	HIPCHK(hipMalloc(&d_jobs_, jobs_bytes_));
	HIPCHK(hipHostMalloc(&h_jobs_, jobs_bytes_, hipHostMallocPortable));
	memset(h_jobs_, 0, jobs_bytes_);

	fill_jobs();
	return 0;
}

// (Re)writes the job tables from plan_: geometry, band addresses and quantizer parameters.
void EncodeBatch::fill_jobs()
{
	for (int i = 0; i < n_; i++) fill_frame_jobs(i);
}
void EncodeBatch::fill_frame_jobs(int i)
{
	const FramePlan &plan = frame_plan(i);              // (the geometry is plan_'s; the divisors are the frame's own)
	const bool bayer = plan.pixel_kind == PIX_BYR4 || plan.pixel_kind == PIX_BYR5;
	const int nch = plan.num_channels, mpq = plan.midpoint_prequant;
	EncJobs j = enc_jobs_at(h_jobs_, n_, nch);
	{
		int16_t *base = d_coeff_ + (size_t)i * plan.coeff_elems;
		const uint8_t *frame = d_in_ + frame_bytes_ * i;
		const Level1 l1 = level1_of(plan, base);
		fill_fwd_yuv_job(j.yuv[i], frame, in_pitch_, plan.width, plan.height, plan.display_height, plan.pixel_kind, plan.precision, l1, mpq, plan.interlaced);
		if (bayer) {
			const int ppitch = plan.ch[0].band[0][0].pitch * 2;
			dev::BayerJob &bj = j.bayer[i];
			bj.in = (const uint16_t *)frame; bj.in_pitch = in_pitch_ / 2;
			bj.width = plan.width; bj.height = plan.height; bj.display_height = plan.display_height;
			bj.out_pitch = ppitch; bj.curve = d_curve_; bj.order = 0; bj.precision = plan.precision; bj.packed12 = plan.pixel_kind == PIX_BYR5;
			for (int c = 0; c < 4; c++) {
				bj.out[c] = d_planes_ + ((size_t)i * 4 + c) * plane_elems_;
				fill_fwd_plane_job(j.l1[(size_t)i * nch + c], bj.out[c], ppitch, plan.ch[c].width, plan.ch[c].height, plan.prescale[0], fwd_bands(l1, c), mpq);
			}
		}
		if (enc_packed16(plan.pixel_kind))
			for (int c = 0; c < nch; c++) {
				dev::FwdPlaneJob &p = j.l1[(size_t)i * nch + c];
				fill_fwd_plane_job(p, nullptr, 0, plan.ch[c].width, plan.ch[c].height, plan.prescale[0], fwd_bands(l1, c), mpq);
				fill_packed16_loader(p, frame, in_pitch_, plan.pixel_kind, plan.encoded_format, plan.color_matrix, plan.width, plan.height, plan.precision, plan.display_height, nch, c);
			}
		for (int lv = 1; lv < 3; lv++)
			for (int c = 0; c < nch; c++) {
				const BandDesc &src = plan.ch[c].band[lv - 1][0];
				fill_fwd_plane_job((lv == 1 ? j.l2 : j.l3)[(size_t)i * nch + c], base + src.offset, src.pitch, src.width, src.height, plan.prescale[lv], fwd_bands(base, plan.ch[c].band[lv]), mpq);
			}
	}
	jobs_dirty_ = true;
}

// New quantizer tables for the frames encoded from now on (rate feedback re-derives them per frame: quantize.c:186, :2865): the band
// geometry is unchanged, only the divisors in the job tables and in the sample headers move.
int EncodeBatch::update_quant(const FramePlan &plan)
{
	(void)hipSetDevice(device_);
	if (plan.coeff_elems != plan_.coeff_elems || plan.num_channels != plan_.num_channels) return -1;
	if (stream_) HIPCHK(hipStreamSynchronize((hipStream_t)stream_));      // the pinned job table may still be in flight
	plan_ = plan; frame_plans_.clear();
	fill_jobs();
	if (ent_ready_) ent_.set_plan(plan);
	return 0;
}

// Frame i's divisors alone: its rows of the job tables are rewritten, the others keep theirs.  The sample header is the caller's (GpuEntropyEncoder::set_plan +
// set_frame_header); the pinned job table must not be in flight (the frame queue rewrites it between the rounds of a pass, behind a drained stream).
int EncodeBatch::set_frame_quant(int i, const FramePlan &plan)
{
	if (i < 0 || i >= n_ || plan.coeff_elems != plan_.coeff_elems || plan.num_channels != plan_.num_channels) return -1;
	if (frame_plans_.empty()) frame_plans_.assign((size_t)n_, plan_);
	frame_plans_[i] = plan;
	fill_frame_jobs(i);
	return 0;
}

int EncodeBatch::prepare_entropy(size_t sample_cap)
{
	int rc = ent_.prepare(plan_, n_, d_coeff_, plan_.coeff_elems, sample_cap, stream_);
	ent_ready_ = rc == 0;
	if (ent_ready_) fill_block_lists();
	// the level-1 bands can be counted while levels 2 and 3 are still being transformed (measured in round 3 against one launch behind level 3: + 2.8 %)
	if (ent_ready_) ent_.set_level1_event(evl_[0]);
	return rc;
}

// Where the forward strip kernel leaves the block lists of the level-1 bands (the entropy stage owns the buffers: GpuEntropyEncoder::prepare).
void EncodeBatch::fill_block_lists()
{
	EncJobs j = enc_jobs_at(h_jobs_, n_, plan_.num_channels);
	int mask_base[kMaxChannels][kNumBands];
	block_list_layout(plan_, mask_base);
	static_assert((int)kBlockChunkCols == (int)dev::FWD_CHUNK_COLS, "one chunk geometry");
	for (int i = 0; i < n_; i++) {
		dev::FwdBlockLists &l = j.yuv[i].lists;
		const bool on = ent_ready_ && ent_.block_slots();
		l.blocks = on ? (uint4 *)ent_.block_slots() : nullptr;
		l.masks = on ? ent_.block_masks(i) : nullptr;
		l.base = d_coeff_;                               // (block slots are numbered over the whole batch's pyramids, as the entropy stage's segment jobs address them)
		for (int c = 0; c < 3; c++) for (int b = 0; b < 4; b++) l.mask_base[c][b] = mask_base[c][b];
	}
	jobs_dirty_ = true;
}

int EncodeBatch::sync_jobs()
{
	(void)hipSetDevice(device_);
	if (!jobs_dirty_) return 0;
	HIPCHK(hipMemcpyAsync(d_jobs_, h_jobs_, jobs_bytes_, hipMemcpyHostToDevice, (hipStream_t)stream_));
	jobs_dirty_ = false;
	return 0;
}

// frames from this size on are staged in pieces (below it the extra calls cost more than the overlap gives); CFHD_AMD_STAGE_MIN_BYTES: tests lower it
static size_t stage_piece_min_bytes() { static const size_t v = [] { const char *e = getenv("CFHD_AMD_STAGE_MIN_BYTES") /* test hook: pieces at the small frames of the CPU suite too */; return e ? (size_t)atoll(e) : ((size_t)1 << 20); }(); return v; }

// The first row in memory of a frame handed over with `pitch`, and in *pitch the (positive) distance its rows are walked at: upload_frame and upload_frame_device.
static const uint8_t *frame_first_row(const FramePlan &plan_, int in_pitch_, int in_rows_, const void *frame, int *pitch_io)
{
	const uint8_t *src = (const uint8_t *)frame;
	int pitch = *pitch_io;
	if (plan_.pixel_kind == PIX_BYR4) {
		// The reference reads a BYR4 frame as tightly packed rows whatever pitch it was given (frame.c:5376-5377: line1 = data + row * width * 4,
		// line2 = line1 + width * 2, in 16-bit words of the component plane width); only the sign of the pitch moves the start (encoder.c:1957,
		// with the pitch doubled by SampleEncoder.cpp:494 and the display height of the component planes).  Same bytes here.
		if (pitch < 0) src += (ptrdiff_t)(plan_.display_height - 1) * 2 * pitch;
		pitch = in_pitch_;
	}
	if (plan_.pixel_kind == PIX_BYR5) pitch = in_pitch_;      // frame.c:5515 walks the frame as tightly packed row pairs of width * 4 * 3 / 2 bytes, whatever the pitch
	if (plan_.pixel_kind == PIX_AV28) {      // frame.c:13179-13186: likewise; a negative pitch still moves the start (encoder.c:1957)
		if (pitch < 0) src += (ptrdiff_t)(plan_.display_height - 1) * pitch;
		pitch = in_pitch_;
	}
	if (pitch < 0) { src += (ptrdiff_t)(in_rows_ - 1) * pitch; pitch = -pitch; }     // encoder.c:1957
	*pitch_io = pitch;
	return src;
}

// upload_frame for a frame that lies in HBM on the batch's device: the same start and pitch, one strided device-to-device copy into the frame's slot on the batch's
// stream, no staging.  The source is the caller's until the stream has drained.
int EncodeBatch::upload_frame_device(int i, const void *d_frame, int pitch)
{
	(void)hipSetDevice(device_);
	if (i < 0 || i >= n_ || !d_frame) return -1;
	const uint8_t *src = frame_first_row(plan_, in_pitch_, in_rows_, d_frame, &pitch);
	if (pitch < in_pitch_) return -1;
	HIPCHK(hipMemcpy2DAsync(d_in_ + frame_bytes_ * i, (size_t)in_pitch_, src, (size_t)pitch, (size_t)in_pitch_, (size_t)in_rows_, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
	return 0;
}

// ---- frames from planar tensors in device memory (k_enc_collect)
int CollectTimes::record(void *stream, bool end)
{
	const size_t at = 2 * (size_t)recorded + (end ? 1 : 0);
	while (ev.size() <= at) { hipEvent_t e = nullptr; HIPCHK(hipEventCreate(&e)); ev.push_back((void *)e); }
	HIPCHK(hipEventRecord((hipEvent_t)ev[at], (hipStream_t)stream));
	if (end) recorded++;
	return 0;
}
void CollectTimes::resolve()
{
	if (!open) return;
	open = false; ms = 0;
	for (int k = 0; k < in_pass; k++) {
		float one = 0;
		if (hipEventElapsedTime(&one, (hipEvent_t)ev[2 * (size_t)k], (hipEvent_t)ev[2 * (size_t)k + 1]) == hipSuccess) ms += one; else (void)hipGetLastError();
	}
	in_pass = 0;
}
void CollectTimes::release()
{
	for (void *e : ev) if (e) (void)hipEventDestroy((hipEvent_t)e);
	ev.clear(); recorded = in_pass = 0; open = false; ms = 0;
}

// The gates and the launch of EncodeBatch:: / GopBatch::upload_frames_device_planar: `slots` holds the batch's `nframes` packed frames, frame_bytes apart, `rows` rows of
// 6 x width bytes back to back (RG48; checked here).  Frame slots, widths and the caller's geometry together put every row of either side on a 16-byte boundary and
// make it a whole number of the kernel's groups of eight pixels (cfhd_collect_kernels.h).
// A BYR4 batch (width: the plan's, photosite quads; rows: the mosaic's, 2 x display height; slot rows of 4 x width bytes) takes the BAYER_* layouts and no other:
// four planes of rows / 2 rows of `width` elements through k_enc_collect_bayer, the same gates over its own geometry.
// A packed 4:2:2 batch takes the YUV422_* layouts (k_enc_collect_yuv422), a b64a, BGRA or BGRa batch the RGBA_* ones (k_enc_collect_rgba), each with gates of its own below.
static int collect_planar_frames(int pixel_kind, uint8_t *slots, size_t frame_bytes, int slot_pitch, int width, int rows, int nframes, int first, int count,
                                 const void *d_frames, size_t frame_stride, int row_pitch, int layout, void *stream, CollectTimes &times)
{
	auto refuse = [](const char *text) { g_err = text; return -1; };
	const bool bayer = pixel_kind == PIX_BYR4;
	if (pixel_kind == PIX_BYR5) return refuse("frames from planar tensors: BYR5 mosaics are not served (BYR4 mosaics are, from four planes)");
	if (bayer && !dev::collect_is_bayer(layout)) return refuse("frames from planar tensors: a BYR4 batch takes the four planes of a mosaic (the BAYER layouts) and no other layout");
	// A packed 4:2:2 batch (YUY2, 2vuy, YU64; width and rows: the frame's; slot rows of 2 x or 4 x width bytes) takes the YUV422_* layouts: a luma plane and two chroma
	// planes of half the width through k_enc_collect_yuv422.  To every other batch but a Bayer one those layouts are named as what they are.
	if (dev::collect_is_yuv422(layout)) {
		if (pixel_kind != PIX_YUY2 && pixel_kind != PIX_2VUY && pixel_kind != PIX_YU64) return refuse("frames from planar tensors: the 4:2:2 plane layouts serve batches whose input is YUY2, 2vuy or YU64");
		const bool words = pixel_kind == PIX_YU64;
		if (layout == dev::COLLECT_YUV422_U8 && words) return refuse("frames from planar tensors: YUV422_U8 serves the 8-bit inputs YUY2 and 2vuy; a YU64 batch takes YUV422_U16");
		if (layout == dev::COLLECT_YUV422_U16 && !words) return refuse("frames from planar tensors: YUV422_U16 serves YU64; a YUY2 or 2vuy batch takes YUV422_U8");
		if (count < 1 || first < 0 || first > nframes - count) return refuse("frames from planar tensors: the run of frames leaves the batch");
		if (!d_frames) return refuse("frames from planar tensors: no pointer");
		if (((uintptr_t)d_frames | frame_stride | (size_t)(unsigned)row_pitch) & 15) return refuse("frames from planar tensors: pointer, frame stride and row pitch are multiples of 16");
		if (row_pitch & 31) return refuse("frames from planar tensors: the row pitch of a 4:2:2 plane layout is a multiple of 32 (the chroma planes' is half of it)");
		if (row_pitch < 0 || (long long)row_pitch < (long long)width * dev::collect_yuv422_element_bytes(layout)) return refuse("frames from planar tensors: a row pitch below the luma row of the 4:2:2 plane layout (width x element size)");
		if (frame_stride < 2 * (size_t)rows * (size_t)row_pitch) return refuse("frames from planar tensors: a frame stride below the three planes of the 4:2:2 layout (2 x height x row pitch)");
		if ((width & 15) || slot_pitch != (words ? 4 : 2) * width || frame_bytes != (size_t)slot_pitch * rows || (((uintptr_t)slots | frame_bytes) & 15) || count > 65535 /* blockIdx.y */)
			return refuse("frames from planar tensors: frame slots the 4:2:2 collect kernel does not take");
		int rc = times.record(stream, false);
		if (rc) return rc;
		(void)hipGetLastError();
		dev::k_enc_collect_yuv422<<<dim3(dev::enc_collect_pieces(rows), (unsigned)count), dev::ENC_COLLECT_THREADS, 0, (hipStream_t)stream>>>(
			(const uint8_t *)d_frames, frame_stride, row_pitch, rows, width, slots + frame_bytes * (size_t)first, frame_bytes, layout,
			words ? dev::COLLECT_ORDER_YU64 : (pixel_kind == PIX_2VUY ? dev::COLLECT_ORDER_2VUY : dev::COLLECT_ORDER_YUY2));
		HIPCHK(hipGetLastError());
		return times.record(stream, true);
	}
	// A b64a, BGRA or BGRa batch (width and rows: the frame's; slot rows of 8 x or 4 x width bytes, a BGRA slot bottom row first) takes the RGBA_* layouts: four planes
	// R, G, B, A, top row first, through k_enc_collect_rgba.  To every other batch those layouts are what they were before they existed.
	if (dev::collect_is_rgba(layout) && (pixel_kind == PIX_B64A || pixel_kind == PIX_BGRA || pixel_kind == PIX_BGRa)) {
		const bool words = pixel_kind == PIX_B64A;
		if (layout == dev::COLLECT_RGBA_U8 && words) return refuse("frames from planar tensors: RGBA_U8 serves the 8-bit inputs BGRA and BGRa; a b64a batch takes RGBA_U16");
		if (layout == dev::COLLECT_RGBA_U16 && !words) return refuse("frames from planar tensors: RGBA_U16 serves b64a; a BGRA or BGRa batch takes RGBA_U8");
		if (count < 1 || first < 0 || first > nframes - count) return refuse("frames from planar tensors: the run of frames leaves the batch");
		if (!d_frames) return refuse("frames from planar tensors: no pointer");
		if (((uintptr_t)d_frames | frame_stride | (size_t)(unsigned)row_pitch) & 15) return refuse("frames from planar tensors: pointer, frame stride and row pitch are multiples of 16");
		if (row_pitch < 0 || (long long)row_pitch < (long long)width * dev::collect_rgba_element_bytes(layout)) return refuse("frames from planar tensors: a row pitch below the plane row of the RGBA layout (width x element size)");
		if (frame_stride < 4 * (size_t)rows * (size_t)row_pitch) return refuse("frames from planar tensors: a frame stride below four planes of the RGBA layout (4 x height x row pitch)");
		if (slot_pitch != (words ? 8 : 4) * width || frame_bytes != (size_t)slot_pitch * rows || (((uintptr_t)slots | frame_bytes | (size_t)slot_pitch) & 15) || count > 65535 /* blockIdx.y */)
			return refuse("frames from planar tensors: frame slots the RGBA collect kernel does not take");
		int rc = times.record(stream, false);
		if (rc) return rc;
		(void)hipGetLastError();
		dev::k_enc_collect_rgba<<<dim3(dev::enc_collect_pieces(rows), (unsigned)count), dev::ENC_COLLECT_THREADS, 0, (hipStream_t)stream>>>(
			(const uint8_t *)d_frames, frame_stride, row_pitch, rows, width, slots + frame_bytes * (size_t)first, frame_bytes, layout,
			words ? dev::COLLECT_ORDER_B64A : (pixel_kind == PIX_BGRA ? dev::COLLECT_ORDER_BGRA : dev::COLLECT_ORDER_BGRa));
		HIPCHK(hipGetLastError());
		return times.record(stream, true);
	}
	if (!bayer && pixel_kind != PIX_RG48) return refuse(dev::collect_is_bayer(layout) ? "frames from planar tensors: the batch's input is not BYR4" : "frames from planar tensors: the batch's input is not RG48");
	if (!bayer && layout != dev::COLLECT_PLANAR_U16 && layout != dev::COLLECT_PLANAR_F16 && layout != dev::COLLECT_PLANAR_F32) return refuse("frames from planar tensors: unknown layout");
	if (count < 1 || first < 0 || first > nframes - count) return refuse("frames from planar tensors: the run of frames leaves the batch");
	if (!d_frames) return refuse("frames from planar tensors: no pointer");
	if (((uintptr_t)d_frames | frame_stride | (size_t)(unsigned)row_pitch) & 15) return refuse("frames from planar tensors: pointer, frame stride and row pitch are multiples of 16");
	const int elt = layout == dev::COLLECT_PLANAR_F32 || layout == dev::COLLECT_BAYER_F32 ? 4 : 2;
	if (row_pitch < 0 || (long long)row_pitch < (long long)width * elt) return refuse("frames from planar tensors: a row pitch below width x element size");
	if (bayer) {
		const int quad_rows = rows / 2;
		if (frame_stride < 4 * (size_t)quad_rows * (size_t)row_pitch) return refuse("frames from planar tensors: a frame stride below four planes (4 x height / 2 x row pitch)");
		if ((width & 7) || (rows & 1) || slot_pitch != 4 * width || frame_bytes != (size_t)slot_pitch * rows || (((uintptr_t)slots | frame_bytes) & 15) || count > 65535 /* blockIdx.y */)
			return refuse("frames from planar tensors: frame slots the Bayer collect kernel does not take");
		int rc = times.record(stream, false);
		if (rc) return rc;
		(void)hipGetLastError();
		dev::k_enc_collect_bayer<<<dim3(dev::enc_collect_pieces(quad_rows), (unsigned)count), dev::ENC_COLLECT_THREADS, 0, (hipStream_t)stream>>>(
			(const uint8_t *)d_frames, frame_stride, row_pitch, quad_rows, width, slots + frame_bytes * (size_t)first, frame_bytes, dev::collect_bayer_element(layout));
		HIPCHK(hipGetLastError());
		return times.record(stream, true);
	}
	if (frame_stride < 3 * (size_t)rows * (size_t)row_pitch) return refuse("frames from planar tensors: a frame stride below three planes (3 x height x row pitch)");
	if ((width & 7) || slot_pitch != 6 * width || frame_bytes != (size_t)slot_pitch * rows || (((uintptr_t)slots | frame_bytes) & 15) || count > 65535 /* blockIdx.y */)
		return refuse("frames from planar tensors: frame slots the collect kernel does not take");
	int rc = times.record(stream, false);
	if (rc) return rc;
	(void)hipGetLastError();
	dev::k_enc_collect<<<dim3(dev::enc_collect_pieces(rows), (unsigned)count), dev::ENC_COLLECT_THREADS, 0, (hipStream_t)stream>>>(
		(const uint8_t *)d_frames, frame_stride, row_pitch, rows, width, slots + frame_bytes * (size_t)first, frame_bytes, layout);
	HIPCHK(hipGetLastError());
	return times.record(stream, true);
}

int EncodeBatch::upload_frames_device_planar(int first, int count, const void *d_frames, size_t frame_stride, int row_pitch, int layout)
{
	(void)hipSetDevice(device_);
	return collect_planar_frames(plan_.pixel_kind, d_in_, frame_bytes_, in_pitch_, plan_.width, in_rows_, n_, first, count, d_frames, frame_stride, row_pitch, layout, stream_, collect_);
}

// Frame i as the batch holds it, in its packed input format: in_rows_ rows of in_pitch_ bytes (av28: the frame's one block), behind whatever the stream holds.
int EncodeBatch::download_input_frame(int i, void *out, int pitch)
{
	(void)hipSetDevice(device_);
	if (i < 0 || i >= n_ || !out || pitch < in_pitch_) return -1;
	HIPCHK(hipMemcpy2DAsync(out, (size_t)pitch, d_in_ + frame_bytes_ * i, (size_t)in_pitch_, (size_t)in_pitch_, (size_t)in_rows_, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
	return 0;
}

int EncodeBatch::upload_frame(int i, const void *frame, int pitch)
{
	(void)hipSetDevice(device_);
	if (i < 0 || i >= n_) return -1;
	const uint8_t *src = frame_first_row(plan_, in_pitch_, in_rows_, frame, &pitch);
	if (pitch >= in_pitch_ && host_buffer_is_registered(src, (size_t)pitch * (in_rows_ - 1) + in_pitch_)) {
		// a buffer the caller registered: DMA straight out of it (the frame is borrowed until the encode completes, as in the reference)
		HIPCHK(hipMemcpy2DAsync(d_in_ + frame_bytes_ * i, (size_t)in_pitch_, src, (size_t)pitch, (size_t)in_pitch_, (size_t)in_rows_, hipMemcpyHostToDevice, (hipStream_t)stream_));
		return 0;
	}
	// a plain buffer: staged through pinned memory, in a few pieces so that the DMA of a piece runs beside the CPU copy of the next (a 1080p frame: 4 MB, 0.2 ms of
	// memcpy and as much of PCIe -- one after the other they were two thirds of a synchronous CFHD_EncodeSample call: 2350 -> 2820 fps).  Only where one caller waits for one
	// frame (set_stage_pieces: the handles of CFHD_EncodeSample / CFHD_DecodeSample): pool workers and gathered decoders run many such copies side by side already, and
	// the extra runtime calls cost them 15-20 % (measured, profiles/r04_j_*).
	const int pieces = frame_bytes_ >= stage_piece_min_bytes() ? stage_pieces_ : 1;
	uint8_t *dst = h_in_ + frame_bytes_ * i;
	for (int k = 0; k < pieces; k++) {
		const int r0 = (int)((long long)in_rows_ * k / pieces), r1 = (int)((long long)in_rows_ * (k + 1) / pieces);
		if (r1 <= r0) continue;
		const size_t off = (size_t)r0 * in_pitch_, bytes = (size_t)(r1 - r0) * in_pitch_;
		if (pitch == in_pitch_) memcpy(dst + off, src + (size_t)r0 * pitch, bytes);
		else for (int r = r0; r < r1; r++) memcpy(dst + (size_t)r * in_pitch_, src + (size_t)r * pitch, (size_t)in_pitch_);
		HIPCHK(hipMemcpyAsync(d_in_ + frame_bytes_ * i + off, dst + off, bytes, hipMemcpyHostToDevice, (hipStream_t)stream_));
	}
	return 0;
}

// The whole batch from host memory, asynchronous on the batch's stream (the frame queue fed from the host: cfhd_amd_batch_submit_host).
int EncodeBatch::upload_frames(const void *frames, size_t frame_stride, int pitch)
{
	(void)hipSetDevice(device_);
	if (!frames) return -1;
	if (plan_.pixel_kind == PIX_AV28 && pitch >= 0) pitch = in_pitch_;      // (ignored: upload_frame)
	if (pitch == in_pitch_ && frame_stride == frame_bytes_ && plan_.pixel_kind != PIX_BYR4 && plan_.pixel_kind != PIX_BYR5 && host_buffer_is_registered(frames, frame_bytes_ * (size_t)n_)) {
		HIPCHK(hipMemcpyAsync(d_in_, frames, frame_bytes_ * (size_t)n_, hipMemcpyHostToDevice, (hipStream_t)stream_));
		return 0;
	}
	if (n_ > 8 && pitch >= in_pitch_ && plan_.pixel_kind != PIX_BYR4 && plan_.pixel_kind != PIX_BYR5 && !host_buffer_is_registered(frames, 1)) {
		// plain memory, many frames: staged into the batch's pinned memory by a few threads side by side (one thread copies 4 MB in ~0.3 ms: 128 frames one after the
		// other were 40 ms of a pass), then ONE copy to the device
		const int nt = n_ < 8 ? n_ : 8;
		std::atomic<int> next(0);
		auto work = [&] {
			for (int i; (i = next.fetch_add(1)) < n_;) {
				const uint8_t *src = (const uint8_t *)frames + frame_stride * (size_t)i; uint8_t *dst = h_in_ + frame_bytes_ * (size_t)i;
				if (pitch == in_pitch_) memcpy(dst, src, frame_bytes_);
				else for (int r = 0; r < in_rows_; r++) memcpy(dst + (size_t)r * in_pitch_, src + (size_t)r * pitch, (size_t)in_pitch_);
			}
		};
		std::vector<std::thread> pool;
		for (int k = 1; k < nt; k++) pool.emplace_back(work);
		work();
		for (auto &t : pool) t.join();
		HIPCHK(hipMemcpyAsync(d_in_, h_in_, frame_bytes_ * (size_t)n_, hipMemcpyHostToDevice, (hipStream_t)stream_));
		return 0;
	}
	for (int i = 0; i < n_; i++) { const int rc = upload_frame(i, (const uint8_t *)frames + frame_stride * (size_t)i, pitch); if (rc) return rc; }
	return 0;
}

// Levels 2 and 3 in the register-strip kernels: one launch per run of equally wide channels (luma | both chroma planes of 4:2:2 | all planes
// of 4:4:4 / Bayer).  false: some channel's geometry is outside what the strip kernels serve (or CFHD_AMD_PLANES=tile) -> tiled kernel.
// The register-strip kernels are the throughput shape: a wave walks down its strip of the plane row by row, so a launch lasts at least one
// such walk (about 80 us at 1080p) however few frames it covers, and fills the chip only with a few hundred frames' worth of strips.  The
// LDS-tiled kernels are many short workgroups: 8x faster on a single frame, slower from a hundred-odd frames on.  Measured crossovers at
// 1080p (tools/small_batch_sweep.sh; frames per launch): plane levels 140-230, forward level 1 about 32, inverse level 1 about 12; larger
// frames count in proportion to their area.  CFHD_AMD_PLANES / _FORWARD / _INVERSE = tile | strip force one shape (A/B runs).
static double frames_1080p_equivalent(const FramePlan &plan, int frames) { return (double)frames * plan.width * plan.height / (1920.0 * 1080.0); }
static int shape_override(const char *name)           // 0: by size, 1: tile, 2: strip (read at every launch: tests switch shapes within one process)
{
	const char *e = getenv(name);
	return !e ? 0 : (strcmp(e, "tile") == 0 ? 1 : (strcmp(e, "strip") == 0 ? 2 : 0));
}
static int active_frames(int active, int n) { return active > 0 && active < n ? active : n; }      // frames 0 .. this-1 of a batch of n take part in a launch (set_active(); 0 = all)
static bool planes_as_strips(const FramePlan &plan, int lv /* wavelet index whose bands are produced / consumed */, int frames)
{
	const int forced = shape_override("CFHD_AMD_PLANES");
	// (the crossover was measured on 4:2:2 frames, whose planes add up to twice the picture; the planes of RGB, RGBA and Bayer frames add up to 3, 4 and 4 times plan.width x plan.height)
	double samples = 0.0;
	for (int c = 0; c < plan.num_channels; c++) samples += (double)plan.ch[c].width * plan.ch[c].height;
	if (forced == 1 || (forced == 0 && frames * samples / (2.0 * 1920.0 * 1080.0) < 160.0)) return false;
	for (int c = 0; c < plan.num_channels; c++) {
		const BandDesc &b = plan.ch[c].band[lv][0];
		if (b.width % dev::SBLK || plan.ch[c].band[lv - 1][0].width != 2 * b.width || plan.ch[c].band[lv - 1][0].height != 2 * b.height ||
		    (plan.ch[c].band[lv - 1][0].pitch & 7) || (b.pitch & 7)) return false;
	}
	return true;
}
template <typename F> static void for_channel_runs(const FramePlan &plan, int lv, F f)
{
	for (int c0 = 0; c0 < plan.num_channels;) {
		int nc = 1;
		while (c0 + nc < plan.num_channels && plan.ch[c0 + nc].band[lv][0].width == plan.ch[c0].band[lv][0].width &&
		       plan.ch[c0 + nc].band[lv][0].height == plan.ch[c0].band[lv][0].height) nc++;
		const BandDesc &b = plan.ch[c0].band[lv][0];
		int glog = 0; while ((1 << glog) < b.width / dev::SBLK) glog++;
		// more than 64 blocks of 8 columns: one plane per wave in segments of PLSTEP blocks (the lanes at a segment's ends feed their neighbours)
		const int nblk = b.width / dev::SBLK, nseg = nblk > 64 ? (nblk + dev::PLSTEP - 1) / dev::PLSTEP : 1;
		if (nseg > 1) glog = 6;
		f(c0, nc, glog, b, nseg);
		c0 += nc;
	}
}

// The launch geometry of k_fwd_plane_strip and k_inv_plane_strip for one run of channels (for_channel_runs): strips of SRP band rows, 64 >> glog planes per wave, four waves per workgroup
struct PlaneStrips { int nstrips; unsigned blocks; };
static PlaneStrips plane_strips(int frames, int nc, int glog, int nseg, int band_height)
{
	const int nstrips = (band_height + dev::SRP - 1) / dev::SRP, per_wave = nseg > 1 ? 1 : 64 >> glog, waves = ((frames * nc + per_wave - 1) / per_wave) * nstrips * nseg;
	return { nstrips, (unsigned)((waves + 3) / 4) };
}
// k_fwd_plane over `planes` source planes of width x height samples: one workgroup per tile of the half-size bands
static void launch_fwd_plane_tiles(const dev::FwdPlaneJob *jobs, int width, int height, int planes, hipStream_t st) { dev::k_fwd_plane<<<dim3((width / 2 + dev::TW - 1) / dev::TW, (height / 2 + dev::TH - 1) / dev::TH, planes), dev::NTHREADS, 0, st>>>(jobs); }

// Level 1 of the forward transform: every kernel launch_forward() can pick -- an intra batch's, and a two-frame group's (one launch over both frames: the tile kernels,
// GopPacked16 for the packed-16 loaders) --, and the name a profiler shows it under (level_kernel(), level1_kernel()).  The strip kernels and the LDS-tiled ones produce
// the same coefficients.
enum class FwdL1 { Yuv422, Yuv422Strip, Yuv422StripBlocks, Yuv422StripBlocksDense, FrameYuv422, FrameYuv422Strip, Packed16, Packed16Strip, BayerStrip, BayerUnpack, GopPacked16 };
static const char *const kFwdL1Name[] = {"k_fwd_yuv422", "k_fwd_yuv422_strip", "k_fwd_yuv422_strip_blocks", "k_fwd_yuv422_strip_blocks_dense", "k_fwd_frame_yuv422",
                                         "k_fwd_frame_yuv422_strip", "k_fwd_packed16", "k_fwd_packed16_strip", "k_fwd_bayer_strip", "k_unpack_byr4+k_fwd_plane", "k_fwd_gop_packed16"};
static const char *const kFwdPlaneName[2] = {"k_fwd_plane", "k_fwd_plane_strip"};      // levels 2 and 3: [planes_as_strips()]
static_assert(sizeof(kFwdL1Name) / sizeof(*kFwdL1Name) == (size_t)FwdL1::GopPacked16 + 1, "one name per level-1 kernel");
struct ForwardRoute {
	FwdL1 l1; bool strip_planes[2];                     // [lv - 1]: level lv + 1 runs as k_fwd_plane_strip
	bool block_lists() const { return l1 == FwdL1::Yuv422StripBlocks || l1 == FwdL1::Yuv422StripBlocksDense; }      // the quantized level-1 bands leave as block lists for k_ent_count_blocks
};
template <typename F> static bool every_frame(int n, F ok) { for (int i = 0; i < n; i++) if (!ok(i)) return false; return true; }

// The kernels of the next launch_forward(), from the prepared batch alone: the environment switches, the active frame count and the job table are read here and nowhere else.
ForwardRoute EncodeBatch::forward_route(bool coeffs_needed, int frames) const
{
	static const int blocks_env = [] { const char *e = getenv("CFHD_AMD_BLOCKS"); return e ? atoi(e) : 1; }();      // 0: dense bands and k_ent_count (A/B runs)
	const int act = frames, forced = shape_override("CFHD_AMD_FORWARD"), kind = plan_.pixel_kind, nch = plan_.num_channels;
	const EncJobs j = enc_jobs_at(h_jobs_, n_, nch);
	ForwardRoute r;
	for (int lv = 1; lv < 3; lv++) r.strip_planes[lv - 1] = planes_as_strips(plan_, lv, act);
	// the register-strip kernels pay from 32 frames of 1080p on (CFHD_AMD_FORWARD=tile / strip, for A/B runs: never / wherever the geometry allows)
	const bool strips = forced != 1 && (forced != 0 || frames_1080p_equivalent(plan_, act) >= 32.0);
	const bool yuy2 = kind == PIX_YUY2 || kind == PIX_2VUY, bayer = kind == PIX_BYR4 || kind == PIX_BYR5;
	// 4:2:2 frames of whole 32-pixel blocks whose rows are 16-byte aligned (k_fwd_yuv422_strip, k_fwd_frame_yuv422_strip)
	const bool yuv_strips = strips && plan_.encoded_format == ENC_YUV422 && plan_.width % 32 == 0 &&
	                        every_frame(n_, [&](int i) { return !((uintptr_t)j.yuv[i].in & 15) && !(j.yuv[i].in_pitch & 15); });
	if (bayer) {
		// BYR4 mosaics whose component planes are whole 8-column blocks wide and whose rows are 16-byte aligned; BYR5 and small launches unpack the planes first
		const bool ok = strips && kind == PIX_BYR4 && plan_.width % 8 == 0 && nch == 4 &&
		                every_frame(n_, [&](int i) { return !((uintptr_t)j.bayer[i].in & 15) && !((j.bayer[i].in_pitch * 2) & 15) && j.bayer[i].order == j.bayer[0].order; });
		r.l1 = ok ? FwdL1::BayerStrip : FwdL1::BayerUnpack;
	} else if (strips && is_packed16(kind) && plan_.encoded_format != ENC_YUV422 && plan_.width % 8 == 0 && nch >= 3 && every_frame(n_, [&](int i) {
		// RG48 / b64a frames of whole 8-pixel blocks whose rows are 16-byte aligned
		const dev::FwdPlaneJob &p = j.l1[(size_t)i * nch];
		const uintptr_t frame = (uintptr_t)((const uint16_t *)p.in - packed_word_of_channel(kind, 0));
		return !(frame & 15) && !((p.in_pitch * 2) & 15) && p.layout == dev::FWD_WORDS16 && p.width % 8 == 0; })) r.l1 = FwdL1::Packed16Strip;
	else if (enc_packed16(kind)) r.l1 = FwdL1::Packed16;
	else if (plan_.interlaced) r.l1 = yuv_strips && yuy2 ? FwdL1::FrameYuv422Strip : FwdL1::FrameYuv422;
	else if (!yuv_strips) r.l1 = FwdL1::Yuv422;
	// block lists wherever the 4:2:2 strip kernel runs in front of the GPU entropy stage; their dense rows are written too when something else reads the coefficients
	else if (blocks_env && ent_ready_ && ent_.block_slots() && yuy2) r.l1 = coeffs_needed ? FwdL1::Yuv422StripBlocksDense : FwdL1::Yuv422StripBlocks;
	else r.l1 = FwdL1::Yuv422Strip;
	return r;
}

// The launch of level 1, for intra batches (`frames` active frames) and two-frame groups (2) alike: every FwdL1 kernel and every grid formula is here and nowhere else.
struct FirstLevel {
	int width, height, frames;                                  // the picture (Bayer: its component planes); grid z
	const dev::FwdYuvJob *yuv; const dev::FwdPlaneJob *l1; const dev::BayerJob *bayer;      // job tables (null: the caller has none)
	int nch, pixel_kind;
	int luma_tiles, chroma_tiles;                               // GopPacked16: tiles of a tile row, the planes side by side in gridDim.x
};
static int launch_first_level(FwdL1 k, const FirstLevel &g, hipStream_t st)
{
	static_assert(sizeof(dev::FwdFrameJob) == sizeof(dev::FwdYuvJob) && offsetof(dev::FwdFrameJob, q) == offsetof(dev::FwdYuvJob, q), "the two level-1 jobs share one table");
	const int hw = g.width / 2, hh = g.height / 2, act = g.frames, nch = g.nch;
	const dim3 tiles((hw + dev::TW - 1) / dev::TW, (hh + dev::TH - 1) / dev::TH, act);      // the LDS-tiled kernels: one workgroup per tile of a half-size plane
	auto strips422 = [&](int rows) { return dim3((g.width / 16 + dev::SSEG - 1) / dev::SSEG, (hh + rows - 1) / rows, act); };      // 4:2:2 strips: segments of 124 luma blocks (1984 pixels)
	const int nseg = (g.width / 8 + dev::PSTEP - 1) / dev::PSTEP, nstrips = (hh + dev::PSR - 1) / dev::PSR, waves = act * nseg * nstrips;      // RG48 / b64a / Bayer strips
	const dev::FwdFrameJob *frame = (const dev::FwdFrameJob *)g.yuv;
	// (a kernel without its job table: no route yields one)
	const bool bayer = k == FwdL1::BayerStrip || k == FwdL1::BayerUnpack, planes = bayer || k == FwdL1::Packed16 || k == FwdL1::Packed16Strip || k == FwdL1::GopPacked16;
	if ((planes ? !g.l1 : !g.yuv) || (bayer && !g.bayer)) { g_err = "forward level 1: no job table for the kernel"; return -1; }
	switch (k) {
	case FwdL1::Packed16: dev::k_fwd_packed16<<<dim3(tiles.x * nch, tiles.y, act), dev::NTHREADS, 0, st>>>(g.l1, nch); break;
	case FwdL1::GopPacked16: dev::k_fwd_gop_packed16<<<dim3(g.luma_tiles + 2 * g.chroma_tiles, tiles.y, act), dev::NTHREADS, 0, st>>>(g.l1, g.luma_tiles); break;
	// level 1 straight from the mosaic, every photosite read and curved once, all four component planes from one pass (cfhd_kernels.h k_fwd_bayer_strip)
	case FwdL1::BayerStrip: dev::k_fwd_bayer_strip<<<(waves + 3) / 4, dev::NTHREADS, 0, st>>>(g.l1, g.bayer, act, nseg, nstrips); break;
	case FwdL1::BayerUnpack:
		dev::k_unpack_byr4<<<dim3((hw + dev::NTHREADS - 1) / dev::NTHREADS, g.height, act), dev::NTHREADS, 0, st>>>(g.bayer);      // two quads per thread
		launch_fwd_plane_tiles(g.l1, g.width, g.height, act * nch, st);
		break;
	case FwdL1::Packed16Strip:
		if (g.pixel_kind == PIX_RG48) dev::k_fwd_packed16_strip<3, 3><<<dim3((waves + 3) / 4), dev::NTHREADS, 0, st>>>(g.l1, act, nseg, nstrips);
		else if (nch == 4) dev::k_fwd_packed16_strip<4, 4><<<dim3((waves + 3) / 4), dev::NTHREADS, 0, st>>>(g.l1, act, nseg, nstrips);
		else dev::k_fwd_packed16_strip<4, 3><<<dim3((waves + 3) / 4), dev::NTHREADS, 0, st>>>(g.l1, act, nseg, nstrips);
		break;
	case FwdL1::FrameYuv422Strip: dev::k_fwd_frame_yuv422_strip<<<strips422(dev::SRI), dev::NTHREADS, 0, st>>>(frame); break;
	case FwdL1::FrameYuv422: dev::k_fwd_frame_yuv422<<<dim3((hw + dev::FTW - 1) / dev::FTW, (hh + dev::FRW - 1) / dev::FRW, act), dev::NTHREADS, 0, st>>>(frame); break;
	case FwdL1::Yuv422StripBlocksDense: dev::k_fwd_yuv422_strip_blocks_dense<<<strips422(dev::SRF), dev::NTHREADS, 0, st>>>(g.yuv); break;
	case FwdL1::Yuv422StripBlocks: dev::k_fwd_yuv422_strip_blocks<<<strips422(dev::SRF), dev::NTHREADS, 0, st>>>(g.yuv); break;
	case FwdL1::Yuv422Strip: dev::k_fwd_yuv422_strip<<<strips422(dev::SRF), dev::NTHREADS, 0, st>>>(g.yuv); break;
	case FwdL1::Yuv422: dev::k_fwd_yuv422<<<tiles, dev::NTHREADS, 0, st>>>(g.yuv); break;
	}
	return 0;
}

const char *EncodeBatch::level_kernel(int level, bool coeffs_needed) const
{
	const ForwardRoute r = forward_route(coeffs_needed, active_frames(active_, n_));
	return level > 0 ? kFwdPlaneName[r.strip_planes[level - 1]] : kFwdL1Name[(int)r.l1];
}

int EncodeBatch::launch_forward(bool coeffs_needed, int first, int count)
{
	if (!count) count = active_frames(active_, n_);      // frames 0 .. count-1 of the batch hold frames (set_active)
	if (first < 0 || count < 1 || first + count > n_) return -1;
	(void)hipSetDevice(device_);
	const ForwardRoute r = forward_route(coeffs_needed, count);
	if (ent_ready_) ent_.set_block_lists(r.block_lists());
	int rc = sync_jobs();
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream_;
	const int nch = plan_.num_channels;
	const int act = count;
	EncJobs j = enc_jobs_at(d_jobs_, n_, nch);
	// (a window: every table from its first frame on -- the jobs hold the addresses of their own frames, pyramids and block lists)
	if (j.yuv) j.yuv += first;
	if (j.bayer) j.bayer += first;
	if (j.l1) j.l1 += (size_t)first * nch;
	j.l2 += (size_t)first * nch; j.l3 += (size_t)first * nch;
	(void)hipGetLastError();                            // drop stale sticky errors: the check below is for these launches only
	timed_ = true;
	HIPCHK(hipEventRecord((hipEvent_t)ev0_, st));
	rc = launch_first_level(r.l1, { plan_.width, plan_.height, act, j.yuv, j.l1, j.bayer, nch, plan_.pixel_kind, 0, 0 }, st);
	if (rc) return rc;
	for (int lv = 1; lv < 3; lv++) {
		HIPCHK(hipEventRecord((hipEvent_t)evl_[lv - 1], st));
		const BandDesc &src = plan_.ch[0].band[lv - 1][0];     // luma is the widest plane of the level
		const dev::FwdPlaneJob *jobs = lv == 1 ? j.l2 : j.l3;
		if (r.strip_planes[lv - 1]) {
			for_channel_runs(plan_, lv, [&](int c0, int nc, int glog, const BandDesc &b, int nseg) {
				const PlaneStrips g = plane_strips(act, nc, glog, nseg, b.height);
				dev::k_fwd_plane_strip<<<g.blocks, dev::NTHREADS, 0, st>>>(jobs, act, nch, c0, nc, glog, g.nstrips, 2 * b.width, 2 * b.height, nseg);
			});
			continue;
		}
		launch_fwd_plane_tiles(jobs, src.width, src.height, act * nch, st);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord((hipEvent_t)ev1_, st));
	return 0;
}

int EncodeBatch::download_coeffs()
{
	(void)hipSetDevice(device_);
	HIPCHK(hipMemcpy2DAsync(h_coeff_, (size_t)plan_.final_elems * 2, d_coeff_, (size_t)plan_.coeff_elems * 2,
	                        (size_t)plan_.final_elems * 2, n_, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	return 0;
}

int EncodeBatch::wait()
{
	(void)hipSetDevice(device_);
	HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
	collect_.resolve();
	float ms = 0;
	if (!timed_) return 0;
	timed_ = false;
	if (hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)ev1_) == hipSuccess) kernel_ms_ = ms;
	if (hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)evl_[0]) == hipSuccess) level_ms_[0] = ms;
	if (hipEventElapsedTime(&ms, (hipEvent_t)evl_[0], (hipEvent_t)evl_[1]) == hipSuccess) level_ms_[1] = ms;
	if (hipEventElapsedTime(&ms, (hipEvent_t)evl_[1], (hipEvent_t)ev1_) == hipSuccess) level_ms_[2] = ms;
	return 0;
}

// =============================================================================================
// Decoder outputs: what an output needs (cfhd_device.h OutputRoute), the job of each family, the conversion pass
// =============================================================================================
// The one place that knows what a requested output of a sample means; DecodeBatch (prepare, inverse_route, launch_inverse) and GopBatch (route, fill_jobs,
// launch_inverse; always ENC_YUV422) read the answer and decide nothing about outputs themselves.  Pure: no environment, no batch state, no geometry -- the band-width
// rules of the 16-bit rows are DecodeBatch::prepare's, the widths a caller may ask for are the C ABI's (cfhd_api_decoder.inc yuv422_output_served).
static OutputRoute output_route(int encoded_format, int kind, bool half, bool interlaced)
{
	OutputRoute r; r.work = kind; r.lowpass_kind = kind;
	const bool yuv8 = kind == PIX_YUY2 || kind == PIX_2VUY, rgb32 = kind == PIX_BGRA || kind == PIX_BGRa, rgb16 = is_packed16(kind), rgb8 = dec_rgb8(kind), rgb10 = dec_rgb10(kind);
	auto refuse = [&r](const char *text) { r.refusal = text; return r; };
	static const char *const not_served = "output format not supported by the GPU path yet";
	// BYR4 output of Bayer samples (decoder.c:14738 + bayer.c:13233 GenerateBYR2): the four component planes as 16-bit rows -- the RG48 route with four planes,
	// four words per photosite quad -- then k_bayer_to_byr4
	if (kind == PIX_BYR4) {
		if (encoded_format != ENC_BAYER || half) return refuse("BYR4 output: Bayer samples, full resolution");
		r.jobs = OutJobs::Planes16; r.work = PIX_RG48; r.convert = OutConvert::Byr4;
		return r;
	}
	if (encoded_format == ENC_YUV422) {
		if (!yuv8 && kind != PIX_YU64 && kind != PIX_V210 && !rgb8 && !rgb16) return refuse(not_served);
		// v210 (10-bit 4:2:2, three samples per 32-bit word): the reference's samples are its YU64 words >> 6 (oracle/cfhd_oracle_inv.c orc_inv_spatial_to_v210, pinned on
		// the reference decoder for widths that are multiples of six) -- YU64 rows into the scratch frame (half resolution: by k_half_yu64), packed by k_yu64_to_v210
		if (kind == PIX_V210) { r.work = PIX_YU64; r.convert = OutConvert::V210; r.width_multiple = 6; r.width_refusal = "v210 output: widths that are multiples of 6"; }
		if (half) {
			// the level-1 lowpass planes are the picture: 8-bit 4:2:2 (k_half_yuv422), YU64 words (k_half_yu64), or -- RG24, BGRA / BGRa, RG48, b64a -- k_half_rgb24's modes
			// straight from the planes (frame.c:8504 and its RGB32 branch, an SSE2 loop of 16 pixels; frame.c:9567): no scratch frame, no last level
			r.jobs = OutJobs::HalfYuv;
			if (rgb8 || rgb16) { r.half_mode = kind == PIX_RG24 ? 0 : (kind == PIX_RG48 ? 2 : (kind == PIX_B64A ? 3 : 1)); r.bottom_up = kind == PIX_BGRA; }
			if (rgb32) { r.width_multiple = 16; r.width_refusal = "BGRA / BGRa output of 4:2:2 samples: half widths that are multiples of 16"; }
			return r;
		}
		if (yuv8) return r;                              // (OutJobs::Yuv: the 4:2:2 kernels, interlaced: the inverse frame transform)
		// BGRA / BGRa of progressive samples: the last level with the reference's fused colour conversion (spatial.c:29577, k_inv_yuv422_rgb32)
		if (rgb32 && !interlaced) return r;
		// Everything else is made from 16-bit rows in the scratch frame.  Progressive: the three planes as YU64 words (k_inv_packed16), then RG24 by the reference's scalar
		// conversion (convert.c:11392 ConvertRow16uToDitheredRGB: k_yu64_to_rgb24), RG48 / b64a by bayer.c:11916 Row16uFull2OutputFormat + RGB2YUV.c:1760 (k_yu64_to_rgb16).
		// Interlaced: RG48 / b64a / BGRA / BGRa from the 16-bit rows of the inverse frame transform (decoder.c:26488 -> :22027 TransformInverseFrameToRow16u,
		// k_inv_frame_yuv422_rows16) -- BGRA / BGRa in k_yu64_to_rgb16's 8-bit mode (bayer.c:825), not the fused kernel; YU64, v210 and RG24 have no such rows (the C ABI
		// refuses them, the planes' route does not run on an interlaced sample: inverse_route)
		r.work = PIX_YU64;
		r.jobs = interlaced && (rgb16 || rgb32) ? OutJobs::Yuv : OutJobs::Planes16;
		if (kind == PIX_RG24) r.convert = OutConvert::Rgb24;
		if (rgb16 || rgb32) { r.convert = OutConvert::Rgb16; r.rgb16_mode = kind == PIX_BGRA ? 3 : (kind == PIX_BGRa ? 2 : (kind == PIX_B64A ? 1 : 0)); }
		return r;
	}
	// RGB 4:4:4 and RGBA 4:4:4:4 samples: RG48 and b64a of either (b64a of RGB 4:4:4: a constant alpha word; RG48 of RGBA: the alpha plane left behind), the 8-bit
	// pixels (not RG24 of RGBA), the 10-bit words of RGB 4:4:4
	const bool rgb = encoded_format == ENC_RGB444, rgba = encoded_format == ENC_RGBA4444;
	if (!((rgb16 && (rgb || rgba)) || (rgb8 && (rgb || (rgba && kind != PIX_RG24))) || (rgb10 && rgb))) return refuse(not_served);
	if (!half) { r.jobs = OutJobs::Planes16; return r; }
	r.jobs = OutJobs::HalfPacked;                        // (half_mode 0: k_half_packed16 -- RG48, b64a of RGBA)
	if (rgb8 || rgb10 || (kind == PIX_B64A && rgb)) {    // k_half_rgb (frame.c:7150 ConvertLowpassRGB444ToRGB)
		r.half_mode = rgb8 ? 1 : (rgb10 ? 2 : 3); r.half_bytes = rgb8 ? rgb8_bytes(kind) : 0;
		r.bottom_up = kind == PIX_RG24 || kind == PIX_BGRA; r.big_endian = kind == PIX_R210 || kind == PIX_DPX0;
	}
	return r;
}

// One job of each family (OutJobs) for frame i, into tables that were zeroed: `out` is where the last launch writes the frame -- the output, or the scratch frame of a conversion
static void fill_half_yuv_job(dev::HalfYuvJob &hj, const Level1 &l, const OutputRoute &r, int rows, int matrix, uint8_t *out, int out_pitch)
{
	for (int c = 0; c < 3; c++) { hj.ll[c] = l.band[c][0]; hj.pitch[c] = l.pitch[c]; }
	hj.width = l.width[0]; hj.rows = rows; hj.uyvy = r.work == PIX_2VUY; hj.matrix = matrix;
	hj.mode = r.half_mode; hj.bottom_up = r.bottom_up;
	hj.out = out; hj.out_pitch = out_pitch;
}
static void fill_half_packed_job(dev::HalfPackedJob &hp, const Level1 &l, const OutputRoute &r, int onch, int precision, int rows, int i, uint8_t *out, int out_pitch)
{
	for (int c = 0; c < onch; c++) { hp.ll[c] = l.band[c][0]; hp.word[c] = dec_rgb10(r.work) ? rgb10_shift(r.work, c) : (r.half_mode ? 0 : packed_word_of_channel(r.work, c)); }
	hp.pitch = l.pitch[0]; hp.width = l.width[0]; hp.rows = rows; hp.nch = onch;
	if (r.half_mode) { hp.mode = r.half_mode; hp.bytes = r.half_bytes; hp.bottom_up = r.bottom_up; hp.big_endian = r.big_endian; hp.dither_seed = 0x9E3779B9u * (uint32_t)(i + 1); }      // k_half_rgb
	else { hp.shift = 16 - precision - 2; hp.alpha = r.work == PIX_B64A; }                                                                                                        // k_half_packed16
	hp.out = (uint16_t *)out; hp.out_pitch = out_pitch;
}
// (nch: the planes of the sample, onch: those that reach the pixel -- dec_out_channels)
static void fill_planes16_jobs(dev::InvPlaneJob *jobs, const Level1 &l, const OutputRoute &r, int nch, int onch, int precision, int display_height, int i, uint8_t *out, int out_pitch)
{
	const int k = r.work;
	for (int c = 0; c < onch; c++) {
		dev::InvPlaneJob &p = jobs[c];
		for (int b = 0; b < 4; b++) p.band[b] = l.band[c][b];
		p.band_pitch = l.pitch[c]; p.width = l.width[c]; p.height = l.height[c]; p.descale = 0;
		p.out = dec_plane_out(out, k, c); p.out_pitch = dec_rgb8(k) ? out_pitch : out_pitch / 2;
		p.xstride = dec_stride_of_channel(k, c, onch); p.precision = precision; p.display_height = display_height;
		p.alpha = (k == PIX_B64A || dec_rgb8(k)) && c == 3;
		p.alpha_const = k == PIX_B64A && nch == 3 ? 0xfff0 : 0;
		p.bytes8 = dec_rgb8(k) ? (nch == 4 ? 2 : 1) : 0;        // 2: BGRA / BGRa of an RGBA 4:4:4:4 sample (alpha from the fourth plane, no dither)
		p.bottom_up = k == PIX_RG24 || k == PIX_BGRA; p.dither_seed = 0x9E3779B9u * (uint32_t)(i + 1);
		if (dec_rgb10(k)) { p.out = (int16_t *)out; p.out_pitch = out_pitch / 4; p.bit_shift = rgb10_shift(k, c); p.big_endian = k == PIX_R210 || k == PIX_DPX0; }
	}
}
// (masks / mask_base, the block lists of an intra batch behind its entropy decoder, are DecodeBatch's to add)
static void fill_inv_yuv_job(dev::InvYuvJob &y, const Level1 &l, const OutputRoute &r, int precision, int display_height, int matrix, int i, uint8_t *out, int out_pitch)
{
	for (int c = 0; c < 3; c++) { y.band_pitch[c] = l.pitch[c]; for (int b = 0; b < 4; b++) y.band[c][b] = l.band[c][b]; }
	y.width = l.width[0]; y.height = l.height[0]; y.display_height = display_height;
	y.uyvy = r.work == PIX_2VUY; y.shift = precision - 8; y.dither_seed = 0x9E3779B9u * (uint32_t)(i + 1);
	y.out = out; y.out_pitch = out_pitch;
	y.bottom_up = r.work == PIX_BGRA; y.matrix_601 = matrix >= 2;       // (k_inv_yuv422_rgb32)
	y.masks = nullptr;
}

// The pass behind the last level of `frames` frames from `first` on: the scratch frames (16-bit rows, `width` pixels -- BYR4: photosite quads -- by `rows` rows) into
// the output frames.  Pitches and frame strides in bytes.  matrix: FramePlan::color_matrix; restore: the linear-restore table of BYR4.
static void launch_convert(const OutputRoute &r, const uint8_t *src8, int src_pitch, size_t src_stride, uint8_t *dst, int dst_pitch, size_t dst_stride, int width, int rows,
                           int first, int frames, int matrix, uint32_t seed, const uint16_t *restore, hipStream_t st)
{
	const uint16_t *src = (const uint16_t *)(src8 + src_stride * first);
	dst += dst_stride * first;
	auto grid = [&](int columns) { return dim3((unsigned)((columns + dev::NTHREADS - 1) / dev::NTHREADS), (unsigned)rows, (unsigned)frames); };
	switch (r.convert) {
	case OutConvert::None: break;
	case OutConvert::V210:                               // six pixels per thread
		dev::k_yu64_to_v210<<<grid(width / 6), dev::NTHREADS, 0, st>>>(src, src_pitch / 2, src_stride / 2, (uint32_t *)dst, dst_pitch / 4, dst_stride / 4, width / 6);
		break;
	case OutConvert::Rgb24:                              // a pixel pair per thread
		dev::k_yu64_to_rgb24<<<grid(width / 2), dev::NTHREADS, 0, st>>>(src, src_pitch / 2, src_stride / 2, dst, dst_pitch, dst_stride, width / 2, rows, matrix, seed);
		break;
	case OutConvert::Rgb16:
		dev::k_yu64_to_rgb16<<<grid(width / 2), dev::NTHREADS, 0, st>>>(src, src_pitch / 2, src_stride / 2, (uint16_t *)dst, dst_pitch / 2, dst_stride / 2, width / 2, matrix >= 2, r.rgb16_mode);
		break;
	case OutConvert::Byr4:                               // a photosite quad per thread
		dev::k_bayer_to_byr4<<<grid(width), dev::NTHREADS, 0, st>>>(src, src_pitch / 2, src_stride / 2, (uint16_t *)dst, dst_pitch / 2, dst_stride / 2, width, restore);
		break;
	}
}

// =============================================================================================
// DecodeBatch
// =============================================================================================
DecodeBatch::DecodeBatch() {}
DecodeBatch::~DecodeBatch() { release(); }

void DecodeBatch::release()
{
	(void)hipSetDevice(device_);
	if (stream_) hipStreamSynchronize((hipStream_t)stream_);
	ent_ready_ = false;
	if (d_out_) hipFree(d_out_);
	if (d_tmp_) { hipFree(d_tmp_); d_tmp_ = nullptr; }
	if (d_restore_) { hipFree(d_restore_); d_restore_ = nullptr; }
	if (h_out_) hipHostFree(h_out_);
	if (d_coeff_) hipFree(d_coeff_);
	if (h_coeff_) hipHostFree(h_coeff_);
	if (d_jobs_) hipFree(d_jobs_);
	if (h_jobs_) hipHostFree(h_jobs_);
	if (ev0_) hipEventDestroy((hipEvent_t)ev0_);
	if (ev1_) hipEventDestroy((hipEvent_t)ev1_);
	for (int k = 0; k < 2; k++) if (evl_[k]) { hipEventDestroy((hipEvent_t)evl_[k]); evl_[k] = nullptr; }
	if (evdep_) { hipEventDestroy((hipEvent_t)evdep_); evdep_ = nullptr; }
	for (void *e : piece_ev_) if (e) hipEventDestroy((hipEvent_t)e);
	piece_ev_.clear(); out_pieces_.clear();
	for (int k = 0; k < 3; k++) if (ev2_[k]) { hipEventDestroy((hipEvent_t)ev2_[k]); ev2_[k] = nullptr; }
	if (stream2_) { device_stream_destroy(stream2_); stream2_ = nullptr; }
	if (stream_) device_stream_destroy(stream_);
	d_out_ = h_out_ = nullptr; d_coeff_ = h_coeff_ = nullptr; d_jobs_ = h_jobs_ = nullptr; stream_ = ev0_ = ev1_ = nullptr; n_ = 0;
}

int DecodeBatch::prepare(const FramePlan &plan, int nframes, int out_kind, bool half)
{
	int rc = device_init();
	if (rc) return rc;
	release();
	device_ = device_current(); (void)hipSetDevice(device_);      // (release() went to the device of the buffers it freed)
	const OutputRoute r = output_route(plan.encoded_format, out_kind, half, interlaced_);
	const int out_width = half ? plan.width / 2 : plan.width, work_rows = half ? plan.display_height / 2 : plan.display_height;
	if (r.refusal || out_width % r.width_multiple) { g_err = r.refusal ? r.refusal : r.width_refusal; return -2; }
	// the tail-column rule of the 16-bit rows (k_inv_packed16, the half-resolution kernels of the same outputs) assumes the reference's vector path: bands of 16 columns
	// and more -- the chroma bands where the rows are YU64 words --, the 8-bit pixels of RGB samples in pairs
	const BandDesc &narrowest = plan.ch[r.work == PIX_YU64 ? 1 : 0].band[0][0];
	if ((r.work == PIX_YU64 || plan.encoded_format != ENC_YUV422) && (narrowest.width < 16 || (dec_rgb8(r.work) && narrowest.width % 2))) { g_err = "output format not supported by the GPU path yet"; return -2; }
	plan_ = plan; n_ = nframes; out_kind_ = out_kind; half_ = half; route_ = r;
	HIPCHK((hipError_t)device_stream_create(&stream_));
	HIPCHK(hipEventCreate((hipEvent_t *)&ev0_));
	HIPCHK(hipEventCreate((hipEvent_t *)&ev1_));
	for (int k = 0; k < 2; k++) HIPCHK(hipEventCreate((hipEvent_t *)&evl_[k]));
	for (int k = 0; k < 3; k++) HIPCHK(hipEventCreate((hipEvent_t *)&ev2_[k]));
	// (a batch of the frame queue creates its second stream only for the arrangement that uses it -- CFHD_AMD_TILES_SPLIT=1, launch_inverse --: a stream that is never used
	// still takes its turn when the runtime deals its 4 hardware queues to the streams in creation order)
	{ const char *se = getenv("CFHD_AMD_TILES_SPLIT"); if ((se && se[0] == '1') || !device_streams_are_lean()) HIPCHK((hipError_t)device_stream_create(&stream2_)); }      // (not lean: the C ABI's handles, cfhd_entropy_gpu.h device_streams_lean)
	// The output frames, in the requested kind; behind a conversion the last level writes scratch frames of the working kind instead.  (BYR4: the plan counts photosite
	// quads -- scratch rows of four words per quad, twice as many mosaic rows.)
	const bool convert = r.convert != OutConvert::None, byr4 = r.convert == OutConvert::Byr4;
	out_rows_ = byr4 ? 2 * work_rows : work_rows;
	out_pitch_ = packed_frame_pitch(out_kind, byr4 ? 2 * plan.width : out_width);
	frame_bytes_ = (size_t)out_pitch_ * out_rows_;
	tmp_pitch_ = !convert ? 0 : (byr4 ? plan.width * 8 : packed_frame_pitch(r.work, out_width)); tmp_frame_bytes_ = (size_t)tmp_pitch_ * work_rows;
	if (convert) HIPCHK(hipMalloc((void **)&d_tmp_, tmp_frame_bytes_ * n_));
	if (byr4) {
		std::vector<uint16_t> curve((size_t)1 << kBayerCurveBits);
		build_bayer_linear_restore_curve(curve.data());
		HIPCHK(hipMalloc((void **)&d_restore_, curve.size() * 2));
		HIPCHK(hipMemcpy(d_restore_, curve.data(), curve.size() * 2, hipMemcpyHostToDevice));
	}
	HIPCHK(hipMalloc((void **)&d_out_, frame_bytes_ * n_));
	HIPCHK(hipHostMalloc((void **)&h_out_, frame_bytes_ * n_, hipHostMallocPortable));
	if (r.convert == OutConvert::V210) HIPCHK(hipMemsetAsync(d_out_, 0, frame_bytes_ * n_, (hipStream_t)stream_));      // (row padding beyond the last whole group of 48 pixels stays zero)
	uint8_t *job_out = convert ? d_tmp_ : d_out_;        // where the last-level kernel writes frame i
	const size_t job_frame_bytes = convert ? tmp_frame_bytes_ : frame_bytes_; const int job_pitch = convert ? tmp_pitch_ : out_pitch_;
	HIPCHK(hipMalloc((void **)&d_coeff_, (size_t)plan.coeff_elems * 2 * n_));
	HIPCHK(hipMemsetAsync(d_coeff_, 0, (size_t)plan.coeff_elems * 2 * n_, (hipStream_t)stream_));
	HIPCHK(hipHostMalloc((void **)&h_coeff_, (size_t)plan.final_elems * 2 * n_, hipHostMallocPortable));
	memset(h_coeff_, 0, (size_t)plan.final_elems * 2 * n_);
	jobs_bytes_ = dec_jobs_bytes(n_, plan.num_channels);
	HIPCHK(hipMalloc(&d_jobs_, jobs_bytes_));
	HIPCHK(hipHostMalloc(&h_jobs_, jobs_bytes_, hipHostMallocPortable));
	memset(h_jobs_, 0, jobs_bytes_);

	const int nch = plan.num_channels, onch = dec_out_channels(r.work, plan);
	DecJobs j = dec_jobs_at(h_jobs_, n_, nch);
	for (int i = 0; i < n_; i++) {
		int16_t *base = d_coeff_ + (size_t)i * plan.coeff_elems;
		for (int lv = 2; lv >= 1; lv--)
			for (int c = 0; c < nch; c++) {
				dev::InvPlaneJob &p = (lv == 2 ? j.l3 : j.l2)[(size_t)i * nch + c];
				for (int b = 0; b < 4; b++) p.band[b] = base + plan.ch[c].band[lv][b].offset;
				p.band_pitch = plan.ch[c].band[lv][0].pitch;
				p.width = plan.ch[c].band[lv][0].width; p.height = plan.ch[c].band[lv][0].height;
				p.descale = plan.prescale[lv];                                  // wavelet.c:5685: prescaled levels use the Descale variant
				p.out = base + plan.ch[c].band[lv - 1][0].offset; p.out_pitch = plan.ch[c].band[lv - 1][0].pitch;
				p.xstride = 1; p.precision = 0; p.display_height = 2 * p.height;
			}
		const Level1 l1 = level1_of(plan, base);
		uint8_t *out = job_out + job_frame_bytes * i;
		switch (r.jobs) {                                // the one table the last launch reads
		case OutJobs::HalfYuv: fill_half_yuv_job(j.half[i], l1, r, out_rows_, plan.color_matrix, out, job_pitch); break;
		case OutJobs::HalfPacked: fill_half_packed_job(j.halfp[i], l1, r, onch, plan.precision, out_rows_, i, out, job_pitch); break;
		case OutJobs::Planes16:
			fill_planes16_jobs(&j.l1[(size_t)i * onch], l1, r, nch, onch, plan.precision, plan.display_height, i, out, job_pitch);
			// (BYR4: where the fused last level writes the mosaic itself, past the scratch frame)
			if (byr4) { j.bayer[i].out = (uint16_t *)(d_out_ + frame_bytes_ * i); j.bayer[i].out_pitch = out_pitch_ / 2; j.bayer[i].curve = d_restore_; }
			break;
		case OutJobs::Yuv: {
			fill_inv_yuv_job(j.yuv[i], l1, r, plan.precision, plan.display_height, plan.color_matrix, i, out, job_pitch);
			// (block lists: prepare_entropy() knows the mask buffer)
			int mb[kMaxChannels][kNumBands]; dec_block_list_layout(plan, mb); for (int c = 0; c < 3; c++) for (int b = 0; b < 4; b++) j.yuv[i].mask_base[c][b] = mb[c][b];
			break;
		}
		}
	}
	jobs_dirty_ = true;
	return 0;
}

int DecodeBatch::prepare_entropy(size_t sample_cap)
{
	ent_.set_skip_level1(half_);                         // half resolution never looks at the level-1 highpass bands
	int rc = ent_.prepare(plan_, n_, d_coeff_, plan_.coeff_elems, sample_cap, route_.lowpass_kind, stream_);
	ent_ready_ = rc == 0;
	if (ent_ready_ && h_jobs_) {
		DecJobs j = dec_jobs_at(h_jobs_, n_, plan_.num_channels);
		for (int i = 0; i < n_; i++) j.yuv[i].masks = ent_.block_masks(i);
		jobs_dirty_ = true;
	}
	return rc;
}

int DecodeBatch::sync_jobs()
{
	(void)hipSetDevice(device_);
	if (!jobs_dirty_) return 0;
	HIPCHK(hipMemcpyAsync(d_jobs_, h_jobs_, jobs_bytes_, hipMemcpyHostToDevice, (hipStream_t)stream_));
	jobs_dirty_ = false;
	return 0;
}

void DecodeBatch::clear_host_coeffs(int i) { memset(h_coeff_ + (size_t)i * plan_.final_elems, 0, (size_t)plan_.final_elems * 2); }

int DecodeBatch::upload_coeffs()
{
	(void)hipSetDevice(device_);
	ent_.dense_pyramid_uploaded();                        // (whatever form the last GPU entropy pass left the level-1 bands in: they are dense rows now)
	HIPCHK(hipMemcpy2DAsync(d_coeff_, (size_t)plan_.coeff_elems * 2, h_coeff_, (size_t)plan_.final_elems * 2,
	                        (size_t)plan_.final_elems * 2, n_, hipMemcpyHostToDevice, (hipStream_t)stream_));
	return 0;
}

// The last level of the inverse transform: every kernel launch_inverse() can pick, and the name a profiler shows it under (level_kernel()).  Where a strip kernel and
// an LDS-tiled one serve the same output they produce the same bytes.
enum class InvL1 { Refused, HalfRgb24, HalfRgb, HalfYu64, HalfPacked16, HalfYuv422, FrameRows16, FrameRows16Col, Packed16Strip, BayerStrip, Yuv422Rgb32, Rgb10, Packed16,
                   FrameYuv422StripBlocks, FrameYuv422Strip, FrameYuv422Quad, FrameYuv422, Yuv422StripBlocks, Yuv422Strip, Yuv422 };
static const char *const kInvL1Name[] = {"refused", "k_half_rgb24", "k_half_rgb", "k_half_yu64", "k_half_packed16", "k_half_yuv422", "k_inv_frame_yuv422_rows16", "k_inv_frame_yuv422_rows16_col",
                                         "k_inv_packed16_strip", "k_inv_bayer_strip", "k_inv_yuv422_rgb32", "k_inv_rgb10", "k_inv_packed16", "k_inv_frame_yuv422_strip_blocks", "k_inv_frame_yuv422_strip",
                                         "k_inv_frame_yuv422_quad", "k_inv_frame_yuv422", "k_inv_yuv422_strip_blocks", "k_inv_yuv422_strip", "k_inv_yuv422"};
static const char *const kInvPlaneName[2] = {"k_inv_plane", "k_inv_plane_strip"};      // levels 3 and 2: [planes_as_strips()]
static_assert(sizeof(kInvL1Name) / sizeof(*kInvL1Name) == (size_t)InvL1::Yuv422 + 1, "one name per last-level kernel");
struct InverseRoute {
	InvL1 l1; bool strip_planes[2];                     // [lv - 1]: level lv + 1 runs as k_inv_plane_strip
	// the level-1 highpass bands travel as block lists between the entropy decoder's tile pass and the kernel that gathers them (cfhd_core.h dec_block_list_layout;
	// interlaced: LH and HH as lists, the difference-coded HL dense)
	bool block_lists() const { return l1 == InvL1::Yuv422StripBlocks || l1 == InvL1::FrameYuv422StripBlocks; }
};

// The half-resolution kernel of a 4:2:2 sample's outputs (OutJobs::HalfYuv), for intra batches and two-frame groups
static InvL1 half_yuv_kernel(const OutputRoute &o) { return o.work == PIX_YU64 ? InvL1::HalfYu64 : (o.work == PIX_YUY2 || o.work == PIX_2VUY ? InvL1::HalfYuv422 : InvL1::HalfRgb24); }

// The interlaced row kernels' four-column shape: whole groups of four luma band columns, band rows of whole 8-byte words (the caller answers for 16-byte output rows)
static bool frame_quads_fit(int forced, int band_w, const int pitch[3]) { return forced != 1 && band_w % 4 == 0 && band_w >= 8 && pitch[0] % 4 == 0 && pitch[1] % 4 == 0 && pitch[2] % 4 == 0; }

// The kernels of the next launch_entropy() + launch_inverse(), from the prepared batch alone.  What the output needs is route_'s (output_route); which shape serves it --
// strips against tiles, block lists, quads -- is decided here: the environment switches, the active frame count and the job table are read here and nowhere else.
InverseRoute DecodeBatch::inverse_route() const
{
	const int blocks_env = [] { const char *e = getenv("CFHD_AMD_DEC_BLOCKS"); return e ? atoi(e) : 1; }();      // 0: dense bands (A/B runs; read at every launch: tests switch within one process)
	const int act = active_frames(active_, n_), forced = shape_override("CFHD_AMD_INVERSE"), nch = plan_.num_channels;
	const BandDesc &b = plan_.ch[0].band[0][0];
	const DecJobs j = dec_jobs_at(h_jobs_, n_, nch);
	InverseRoute r;
	for (int lv = 1; lv < 3; lv++) r.strip_planes[lv - 1] = planes_as_strips(plan_, lv, act);
	// the register-strip kernels pay from 12 frames of 1080p on (CFHD_AMD_INVERSE=tile / strip, for A/B runs: never / wherever the geometry allows)
	const bool strips = forced != 1 && (forced != 0 || frames_1080p_equivalent(plan_, act) >= 12.0);
	// ... the fused last level of BYR4 from 4 on: measured at 2, 4, 12 and 32 mosaics of 3840 x 2160 (one 1080p frame's worth of quads each), the pair wins beyond
	// the spread at 2 (0.079 against 0.098 ms: a strip launch has a floor of 0.10 ms) and the fused kernel from 4 on (0.100 against 0.130, 0.156 against 0.379,
	// 0.324 against 0.982 ms)
	const bool bayer_strips = forced != 1 && (forced != 0 || frames_1080p_equivalent(plan_, act) >= 4.0);
	const int pitch[3] = { b.pitch, plan_.ch[1].band[0][0].pitch, plan_.ch[2].band[0][0].pitch };
	auto rows_aligned = [&] { return every_frame(n_, [&](int i) { return !((uintptr_t)j.yuv[i].out & 15) && !(j.yuv[i].out_pitch & 15); }); };      // 16-byte stores
	auto quads = [&] { return frame_quads_fit(forced, b.width, pitch) && rows_aligned(); };
	// 8-bit 4:2:2 pictures behind the chunk-indexed GPU entropy decoder take the level-1 bands as block lists wherever a 4:2:2 strip kernel runs
	const bool lists = blocks_env && ent_ready_ && ent_.block_masks(0) && ent_.chunk_indexed() && (out_kind_ == PIX_YUY2 || out_kind_ == PIX_2VUY) && plan_.encoded_format == ENC_YUV422;
	const int work = route_.work;
	switch (route_.jobs) {
	// half resolution: the last level is not run, the level-1 lowpass planes are the picture
	case OutJobs::HalfYuv: r.l1 = half_yuv_kernel(route_); break;
	case OutJobs::HalfPacked: r.l1 = route_.half_mode ? InvL1::HalfRgb : InvL1::HalfPacked16; break;
	case OutJobs::Planes16:
		// (interlaced samples at full resolution have no planes' route: YU64, v210, RG24 and the 10-bit RGB words are refused at the C ABI)
		if (interlaced_) r.l1 = InvL1::Refused;
		// RG48 / b64a output of whole 8-pixel blocks whose rows are 16-byte aligned (the strip kernel knows the RG48 and b64a pixels only)
		else if (strips && is_packed16(work) && b.width % 4 == 0 && !(work == PIX_B64A && nch == 3) && route_.convert != OutConvert::Byr4 && every_frame(n_, [&](int i) {
			const dev::InvPlaneJob &p = j.l1[(size_t)i * dec_out_channels(work, plan_)];
			const uintptr_t frame = (uintptr_t)((const uint16_t *)p.out - packed_word_of_channel(work, 0));
			return !(frame & 15) && !((p.out_pitch * 2) & 15) && !(p.band_pitch & 3); })) r.l1 = InvL1::Packed16Strip;
		// BYR4 output of a batch that opted in (set_bayer_strips: the queues' Bayer batches, never a handle): the mosaic straight from the last level, no scratch
		// frame and no k_bayer_to_byr4 -- band rows of whole 8-byte words, mosaic rows in 16-byte words
		else if (bayer_strips && bayer_strips_ && route_.convert == OutConvert::Byr4 && b.width % 4 == 0 && every_frame(n_, [&](int i) {
			const dev::InvPlaneJob *p = &j.l1[(size_t)i * nch];
			for (int c = 0; c < nch; c++) if ((p[c].band_pitch & 3) || p[c].width != b.width || p[c].height != b.height) return false;
			return nch == 4 && !((uintptr_t)j.bayer[i].out & 15) && !((j.bayer[i].out_pitch * 2) & 15); })) r.l1 = InvL1::BayerStrip;
		else r.l1 = dec_rgb10(work) ? InvL1::Rgb10 : InvL1::Packed16;
		break;
	case OutJobs::Yuv:
		// interlaced: four band columns per thread with 8-byte loads and 16-byte stores, else the one-column kernel
		if (route_.convert == OutConvert::Rgb16) r.l1 = quads() ? InvL1::FrameRows16 : InvL1::FrameRows16Col;
		else if (dec_rgb8(work)) r.l1 = InvL1::Yuv422Rgb32;
		// 4:2:2 pictures: luma bands of whole 16-column blocks, written in 16-byte words (interlaced: band rows of whole 8-coefficient words too)
		else if (strips && b.width % 16 == 0 && rows_aligned() && (!interlaced_ || !(pitch[0] % 8 || pitch[1] % 8 || pitch[2] % 8)))
			r.l1 = interlaced_ ? (lists ? InvL1::FrameYuv422StripBlocks : InvL1::FrameYuv422Strip) : (lists ? InvL1::Yuv422StripBlocks : InvL1::Yuv422Strip);
		else if (interlaced_) r.l1 = quads() ? InvL1::FrameYuv422Quad : InvL1::FrameYuv422;
		else r.l1 = InvL1::Yuv422;
		break;
	}
	return r;
}

// The launch of the last level, for intra batches (`frames` active frames) and two-frame groups alike: every InvL1 kernel and every grid formula is here and nowhere else.
struct LastLevel {
	int band_w, band_h, out_rows, frames; bool interlaced;      // the luma band of level 1; the rows of a half-resolution output; grid z
	const dev::InvYuvJob *yuv; const dev::InvPlaneJob *l1; const dev::HalfYuvJob *half; const dev::HalfPackedJob *halfp;      // job tables (null: the caller has none)
	int out_channels, words_per_position;                       // of the packed 16-bit outputs
	const dev::InvBayerJob *bayer;                              // beside l1 for k_inv_bayer_strip (null: the caller has none)
};
static int launch_last_level(InvL1 k, const LastLevel &g, uint32_t dither_seed, hipStream_t st)
{
	const dim3 tiles((g.band_w + dev::ITW - 1) / dev::ITW, (g.band_h + dev::ITH - 1) / dev::ITH, g.frames);      // the LDS-tiled kernels: one workgroup per tile, all components
	const int sr = g.interlaced ? dev::SRI : dev::SR;
	const dim3 strips((g.band_w / dev::SBLK + dev::SSEG - 1) / dev::SSEG, (g.band_h + sr - 1) / sr, g.frames);      // the 4:2:2 strip kernels: segments of 124 luma blocks, sr band rows
	auto rows = [&](int cols_per_thread, int nrows) { return dim3((g.band_w / cols_per_thread + dev::NTHREADS - 1) / dev::NTHREADS, nrows, g.frames); };      // the row kernels: one thread per group of band columns
	auto unserved = [] { g_err = "two-frame groups: output not served"; return -1; };      // (a kernel without its job table: GopBatch::route() yields none)
	switch (k) {
	case InvL1::Refused: break;                         // (left by the callers)
	case InvL1::FrameRows16: if (!g.yuv) return unserved(); dev::k_inv_frame_yuv422_rows16<<<rows(4, g.band_h), dev::NTHREADS, 0, st>>>(g.yuv); break;
	case InvL1::FrameRows16Col: if (!g.yuv) return unserved(); dev::k_inv_frame_yuv422_rows16_col<<<rows(2, g.band_h), dev::NTHREADS, 0, st>>>(g.yuv); break;
	// half resolution: the level-1 lowpass planes are the picture, no last level
	case InvL1::HalfRgb24: if (!g.half) return unserved(); dev::k_half_rgb24<<<rows(2, g.out_rows), dev::NTHREADS, 0, st>>>(g.half); break;
	case InvL1::HalfRgb: if (!g.halfp) return unserved(); dev::k_half_rgb<<<rows(1, g.out_rows), dev::NTHREADS, 0, st>>>(g.halfp, dither_seed); break;
	case InvL1::HalfYu64: if (!g.half) return unserved(); dev::k_half_yu64<<<rows(2, g.out_rows), dev::NTHREADS, 0, st>>>(g.half); break;
	case InvL1::HalfPacked16: if (!g.halfp) return unserved(); dev::k_half_packed16<<<rows(8, g.out_rows), dev::NTHREADS, 0, st>>>(g.halfp); break;
	case InvL1::HalfYuv422: if (!g.half) return unserved(); dev::k_half_yuv422<<<rows(8, g.out_rows), dev::NTHREADS, 0, st>>>(g.half); break;
	case InvL1::Packed16Strip: {
		if (!g.l1) return unserved();
		const int nseg = (g.band_w / 4 + dev::PSTEP - 1) / dev::PSTEP, nstrips = (g.band_h + dev::QSR - 1) / dev::QSR, waves = g.frames * nseg * nstrips;
		if (g.out_channels == 4) dev::k_inv_packed16_strip<4><<<(waves + 3) / 4, dev::NTHREADS, 0, st>>>(g.l1, g.frames, nseg, nstrips);
		else dev::k_inv_packed16_strip<3><<<(waves + 3) / 4, dev::NTHREADS, 0, st>>>(g.l1, g.frames, nseg, nstrips);
		break;
	}
	case InvL1::BayerStrip: {
		if (!g.l1 || !g.bayer) return unserved();
		const int nseg = (g.band_w / 4 + dev::PSTEP - 1) / dev::PSTEP, nstrips = (g.band_h + dev::QSR - 1) / dev::QSR, waves = g.frames * nseg * nstrips;
		dev::k_inv_bayer_strip<<<(waves + 3) / 4, dev::NTHREADS, 0, st>>>(g.l1, g.bayer, g.frames, nseg, nstrips);
		break;
	}
	case InvL1::Yuv422Rgb32: if (!g.yuv) return unserved(); dev::k_inv_yuv422_rgb32<<<tiles, dev::NTHREADS, 0, st>>>(g.yuv); break;
	case InvL1::Rgb10: if (!g.l1) return unserved(); dev::k_inv_rgb10<<<tiles, dev::NTHREADS, 0, st>>>(g.l1); break;
	case InvL1::Packed16: if (!g.l1) return unserved(); dev::k_inv_packed16<<<tiles, dev::NTHREADS, 0, st>>>(g.l1, g.out_channels, g.words_per_position, dither_seed); break;
	case InvL1::FrameYuv422StripBlocks: if (!g.yuv) return unserved(); dev::k_inv_frame_yuv422_strip_blocks<<<strips, dev::NTHREADS, 0, st>>>(g.yuv, dither_seed); break;
	case InvL1::FrameYuv422Strip: if (!g.yuv) return unserved(); dev::k_inv_frame_yuv422_strip<<<strips, dev::NTHREADS, 0, st>>>(g.yuv, dither_seed); break;
	case InvL1::FrameYuv422Quad: if (!g.yuv) return unserved(); dev::k_inv_frame_yuv422_quad<<<rows(4, g.band_h), dev::NTHREADS, 0, st>>>(g.yuv, dither_seed); break;
	case InvL1::FrameYuv422: if (!g.yuv) return unserved(); dev::k_inv_frame_yuv422<<<rows(2, g.band_h), dev::NTHREADS, 0, st>>>(g.yuv, dither_seed); break;
	case InvL1::Yuv422StripBlocks: if (!g.yuv) return unserved(); dev::k_inv_yuv422_strip_blocks<<<strips, dev::NTHREADS, 0, st>>>(g.yuv, dither_seed); break;
	case InvL1::Yuv422Strip: if (!g.yuv) return unserved(); dev::k_inv_yuv422_strip<<<strips, dev::NTHREADS, 0, st>>>(g.yuv, dither_seed); break;
	case InvL1::Yuv422: if (!g.yuv) return unserved(); dev::k_inv_yuv422<<<tiles, dev::NTHREADS, 0, st>>>(g.yuv, dither_seed); break;
	}
	return 0;
}

const char *DecodeBatch::level_kernel(int level) const
{
	const InverseRoute r = inverse_route();
	if (level == 0 && route_.convert == OutConvert::Byr4 && r.l1 == InvL1::Packed16) return "k_inv_packed16+k_bayer_to_byr4";      // (the pair behind BYR4; the fused kernel carries its own name)
	return level > 0 ? kInvPlaneName[r.strip_planes[level - 1]] : kInvL1Name[(int)r.l1];
}

int DecodeBatch::launch_entropy()
{
	ent_.set_block_lists(inverse_route().block_lists());
	return ent_.launch();
}

int DecodeBatch::launch_inverse(uint32_t dither_seed)
{
	InverseRoute r = inverse_route();
	// (the level-1 bands of the last entropy pass are block lists: only the kernel that gathers them may run behind it)
	const bool lists = ent_ready_ && ent_.level1_as_block_lists();
	if (lists && !r.block_lists()) { g_err = "the level-1 bands are block lists but the inverse would read them as dense rows"; return -1; }
	if (r.l1 == InvL1::Refused) return -1;
	// (the route is what the next entropy pass would leave; bands that came as dense rows -- upload_coeffs() -- go through the same strip kernel's dense form)
	if (!lists && r.block_lists()) r.l1 = interlaced_ ? InvL1::FrameYuv422Strip : InvL1::Yuv422Strip;
	(void)hipSetDevice(device_);
	const bool jobs_uploaded_now = jobs_dirty_;          // (the upload is queued on `st`: a second stream must not read the tables before it)
	int rc = sync_jobs();
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream_;
	const int nch = plan_.num_channels;
	const int act = active_frames(active_, n_);                    // frames 0 .. act-1 carry pyramids (set_active)
	DecJobs j = dec_jobs_at(d_jobs_, n_, nch);
	(void)hipGetLastError();
	timed_ = true;
	// The entropy decoder may have finished the bands of levels 3 and 2 ahead of the level-1 bands (its tile pass over those is still queued on `st`): then the
	// inverse transforms of levels 3 and 2 run on a second stream beside it, and level 1 waits for both.
	void *l23 = ent_ready_ ? ent_.levels23_event() : nullptr;
	inv_split_ = l23 && stream2_ && !jobs_uploaded_now;
	hipStream_t sl = inv_split_ ? (hipStream_t)stream2_ : st;      // the stream of levels 3 and 2
	if (inv_split_) { HIPCHK(hipStreamWaitEvent(sl, (hipEvent_t)l23, 0)); HIPCHK(hipEventRecord((hipEvent_t)ev2_[0], sl)); }
	HIPCHK(hipEventRecord((hipEvent_t)ev0_, st));
	for (int lv = 2; lv >= 1; lv--) {
		const BandDesc &lb = plan_.ch[0].band[lv][0];
		const dev::InvPlaneJob *jobs = lv == 2 ? j.l3 : j.l2;
		if (r.strip_planes[lv - 1]) {
			for_channel_runs(plan_, lv, [&](int c0, int nc, int glog, const BandDesc &cb, int nseg) {
				const PlaneStrips g = plane_strips(act, nc, glog, nseg, cb.height);
				dev::k_inv_plane_strip<<<g.blocks, dev::NTHREADS, 0, sl>>>(jobs, act, nch, c0, nc, glog, g.nstrips, cb.width, cb.height, nseg);
			});
			HIPCHK(hipEventRecord((hipEvent_t)(inv_split_ ? ev2_[3 - lv] : evl_[2 - lv]), sl));
			continue;
		}
		dim3 grid((lb.width + dev::ITW - 1) / dev::ITW, (lb.height + dev::ITH - 1) / dev::ITH, act * nch);
		dev::k_inv_plane<<<grid, dev::NTHREADS, 0, sl>>>(jobs);
		HIPCHK(hipEventRecord((hipEvent_t)(inv_split_ ? ev2_[3 - lv] : evl_[2 - lv]), sl));
	}
	if (inv_split_) {                                   // level 1 behind the level-1 tiles (stream order) and behind levels 3 and 2 (this wait)
		HIPCHK(hipStreamWaitEvent(st, (hipEvent_t)ev2_[2], 0));
		HIPCHK(hipEventRecord((hipEvent_t)evl_[1], st));
	}
	const BandDesc &b = plan_.ch[0].band[0][0];
	const int onch = dec_out_channels(route_.work, plan_);
	rc = launch_last_level(r.l1, { b.width, b.height, out_rows_, act, interlaced_, j.yuv, j.l1, j.half, j.halfp, onch, dec_words_per_position(route_.work, onch), j.bayer }, dither_seed, st);
	if (rc) return rc;
	if (r.l1 != InvL1::BayerStrip)                      // (the fused last level of BYR4 wrote the mosaic itself)
		launch_convert(route_, d_tmp_, tmp_pitch_, tmp_frame_bytes_, d_out_, out_pitch_, frame_bytes_, half_ ? plan_.width / 2 : plan_.width, half_ ? plan_.display_height / 2 : plan_.display_height,
	               0, act, plan_.color_matrix, dither_seed, d_restore_, st);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord((hipEvent_t)ev1_, st));
	return 0;
}

int DecodeBatch::download_frame(int i, void *out, int pitch)
{
	(void)hipSetDevice(device_);
	if (i < 0 || i >= n_) return -1;
	if (direct_.size() != (size_t)n_) direct_.assign((size_t)n_, 0);
	direct_[i] = 0;
	if (out && pitch >= out_pitch_ && host_buffer_is_registered(out, (size_t)pitch * (out_rows_ - 1) + out_pitch_)) {
		HIPCHK(hipMemcpy2DAsync(out, (size_t)pitch, d_out_ + frame_bytes_ * i, (size_t)out_pitch_, (size_t)out_pitch_, (size_t)out_rows_, hipMemcpyDeviceToHost, (hipStream_t)stream_));
		direct_[i] = 1;
		return 0;
	}
	// a plain buffer: staged through pinned memory; the few frames of a C ABI call come in pieces with an event behind each, so that finish_frame() can copy a piece
	// into the caller's buffer while the DMA of the next is still running (as EncodeBatch::upload_frame does on the way in)
	const int pieces = (n_ <= 8 && frame_bytes_ >= stage_piece_min_bytes()) ? (stage_pieces_ > kMaxOutPieces ? (int)kMaxOutPieces : stage_pieces_) : 1;
	if (out_pieces_.size() != (size_t)n_) out_pieces_.assign((size_t)n_, 0);
	out_pieces_[i] = 0;
	if (stage_pieces_ > 1) {                             // (a batch that stages in pieces puts an event behind every frame it stages, also behind one that is too small to cut: finish_frame() may run before wait())
		if (piece_ev_.size() != (size_t)n_ * kMaxOutPieces) {
			piece_ev_.assign((size_t)n_ * kMaxOutPieces, nullptr);
			for (void *&e : piece_ev_) { hipEvent_t ev; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); e = ev; }
		}
		for (int k = 0; k < pieces; k++) {
			const int r0 = (int)((long long)out_rows_ * k / pieces), r1 = (int)((long long)out_rows_ * (k + 1) / pieces);
			const size_t off = (size_t)r0 * out_pitch_, bytes = (size_t)(r1 - r0) * out_pitch_;
			if (bytes) HIPCHK(hipMemcpyAsync(h_out_ + frame_bytes_ * i + off, d_out_ + frame_bytes_ * i + off, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream_));
			HIPCHK(hipEventRecord((hipEvent_t)piece_ev_[(size_t)i * kMaxOutPieces + k], (hipStream_t)stream_));
		}
		out_pieces_[i] = pieces;
		return 0;
	}
	HIPCHK(hipMemcpyAsync(h_out_ + frame_bytes_ * i, d_out_ + frame_bytes_ * i, frame_bytes_, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	return 0;
}

// The whole batch to host memory, asynchronous on the batch's stream; behind wait() the caller runs finish_frame() for every frame (nothing to do for frames that went
// straight into a registered buffer).
int DecodeBatch::download_frames(void *out, size_t frame_stride, int pitch)
{
	(void)hipSetDevice(device_);
	if (!out) return -1;
	const int act = active_frames(active_, n_);          // frames 0 .. act-1 carry pictures (set_active)
	if (pitch == out_pitch_ && frame_stride == frame_bytes_ && host_buffer_is_registered(out, frame_bytes_ * (size_t)act)) {
		HIPCHK(hipMemcpyAsync(out, d_out_, frame_bytes_ * (size_t)act, hipMemcpyDeviceToHost, (hipStream_t)stream_));
		direct_.assign((size_t)n_, 1);
		return 0;
	}
	if (n_ > 8 && !host_buffer_is_registered(out, 1)) {
		// plain memory, many frames: ONE copy into the batch's pinned memory; finish_frame() copies every frame out behind wait() (the caller runs them on several threads)
		HIPCHK(hipMemcpyAsync(h_out_, d_out_, frame_bytes_ * (size_t)act, hipMemcpyDeviceToHost, (hipStream_t)stream_));
		direct_.assign((size_t)n_, 0);
		out_pieces_.assign((size_t)n_, 0);
		return 0;
	}
	for (int i = 0; i < act; i++) { const int rc = download_frame(i, (uint8_t *)out + frame_stride * (size_t)i, pitch); if (rc) return rc; }
	return 0;
}

// Orders everything queued on this batch's stream from now on behind what the producer stream holds at this moment.
int DecodeBatch::after(void *producer_stream)
{
	(void)hipSetDevice(device_);
	if (!evdep_) { hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); evdep_ = e; }
	HIPCHK(hipEventRecord((hipEvent_t)evdep_, (hipStream_t)producer_stream));
	HIPCHK(hipStreamWaitEvent((hipStream_t)stream_, (hipEvent_t)evdep_, 0));
	return 0;
}

int DecodeBatch::wait()
{
	(void)hipSetDevice(device_);
	HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
	float ms = 0;
	if (!timed_) return 0;
	timed_ = false;
	if (hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)ev1_) == hipSuccess) kernel_ms_ = ms;
	if (inv_split_) {                                   // levels 3 and 2 ran on the second stream: their own events
		if (hipEventElapsedTime(&ms, (hipEvent_t)ev2_[0], (hipEvent_t)ev2_[1]) == hipSuccess) level_ms_[2] = ms;
		if (hipEventElapsedTime(&ms, (hipEvent_t)ev2_[1], (hipEvent_t)ev2_[2]) == hipSuccess) level_ms_[1] = ms;
	} else {
		if (hipEventElapsedTime(&ms, (hipEvent_t)ev0_, (hipEvent_t)evl_[0]) == hipSuccess) level_ms_[2] = ms;
		if (hipEventElapsedTime(&ms, (hipEvent_t)evl_[0], (hipEvent_t)evl_[1]) == hipSuccess) level_ms_[1] = ms;
	}
	if (hipEventElapsedTime(&ms, (hipEvent_t)evl_[1], (hipEvent_t)ev1_) == hipSuccess) level_ms_[0] = ms;
	return 0;
}

int DecodeBatch::finish_frame(int i, void *out, int pitch)
{
	if (i < 0 || i >= n_) return -1;
	if (direct_.size() == (size_t)n_ && direct_[i]) return 0;            // already in the caller's buffer
	const uint8_t *src = h_out_ + frame_bytes_ * i;
	uint8_t *dst = (uint8_t *)out;
	const int pieces = out_pieces_.size() == (size_t)n_ ? out_pieces_[i] : 0;
	if (pieces >= 1) {
		// the frame came down in pieces (download_frame): every piece is copied out as soon as its DMA has finished, beside the DMA of the next one.  (May be
		// called before wait(): the events order it; after wait() they have all fired.)
		(void)hipSetDevice(device_);
		for (int k = 0; k < pieces; k++) {
			const int r0 = (int)((long long)out_rows_ * k / pieces), r1 = (int)((long long)out_rows_ * (k + 1) / pieces);
			HIPCHK(hipEventSynchronize((hipEvent_t)piece_ev_[(size_t)i * kMaxOutPieces + k]));
			if (pitch == out_pitch_) memcpy(dst + (size_t)r0 * out_pitch_, src + (size_t)r0 * out_pitch_, (size_t)(r1 - r0) * out_pitch_);
			else for (int r = r0; r < r1; r++) memcpy(dst + (ptrdiff_t)r * pitch, src + (size_t)r * out_pitch_, (size_t)out_pitch_);
		}
		return 0;
	}
	if (pitch == out_pitch_) memcpy(dst, src, frame_bytes_);
	else for (int r = 0; r < out_rows_; r++) memcpy(dst + (ptrdiff_t)r * pitch, src + (size_t)r * out_pitch_, (size_t)out_pitch_);
	return 0;
}

// =============================================================================================
// GopBatch
// =============================================================================================
namespace {
struct GopJobs {            // layout of a GopBatch's job table: n groups, every row n times as long, group g's entries at g times the row's length of one group
	dev::FwdYuvJob *yuv;        // [2 n]    level 1 of the frames, frame f of group g at 2 g + f
	dev::GopTemporalJob *temp;  // [3 n]    per channel
	dev::FwdPlaneJob *mid;      // [6 n]    w[3] (from the temporal highpass band) and w[4] (from the lowpass band), per channel
	dev::FwdPlaneJob *top;      // [3 n]    w[5]
	dev::InvPlaneJob *itop;     // [3 n]    w[5] -> lowpass band of w[4]
	dev::InvPlaneJob *imid;     // [6 n]    w[4] -> temporal lowpass, w[3] -> temporal highpass
	dev::InvYuvJob *iyuv;       // [2 n]    last level of the frames: k_inv_yuv422 / k_inv_frame_yuv422 / k_inv_yuv422_rgb32 / k_inv_frame_yuv422_rows16(_col)
	dev::InvPlaneJob *l1;       // [2 n * 3] the same as YU64 rows (k_inv_packed16), frame f channel c at 3 f + c
	dev::HalfYuvJob *half;      // [2 n]    half resolution: the level-1 lowpass plane of each frame (k_half_yuv422 / k_half_yu64 / k_half_rgb24)
	dev::FwdPlaneJob *fl1;      // [2 n * 3] level 1 of the frames from the inputs of the packed-16 loaders (k_fwd_gop_packed16), frame f plane c at 3 f + c
	dev::GopQuantJob *tq;       // [3 n]    the lowpass band of w[3] where it is divided and coded (k_gop_quant_lowpass)
};
GopJobs gop_jobs_at(void *base, int n)
{
	GopJobs j;
	j.yuv = (dev::FwdYuvJob *)base; j.temp = (dev::GopTemporalJob *)(j.yuv + 2 * n); j.mid = (dev::FwdPlaneJob *)(j.temp + 3 * n); j.top = j.mid + 6 * n;
	j.itop = (dev::InvPlaneJob *)(j.top + 3 * n); j.imid = j.itop + 3 * n; j.iyuv = (dev::InvYuvJob *)(j.imid + 6 * n);
	j.l1 = (dev::InvPlaneJob *)(j.iyuv + 2 * n); j.half = (dev::HalfYuvJob *)(j.l1 + 6 * n); j.fl1 = (dev::FwdPlaneJob *)(j.half + 2 * n); j.tq = (dev::GopQuantJob *)(j.fl1 + 6 * n);
	return j;
}
size_t gop_jobs_bytes(int n) { return (size_t)n * (2 * sizeof(dev::FwdYuvJob) + 3 * sizeof(dev::GopTemporalJob) + 15 * sizeof(dev::FwdPlaneJob) + 15 * sizeof(dev::InvPlaneJob) + 2 * sizeof(dev::InvYuvJob) + 2 * sizeof(dev::HalfYuvJob) + 3 * sizeof(dev::GopQuantJob)); }
enum { kMaxGridYZ = 65535 };
}

// The forward twin of route(): which kernel transforms the two input frames in one launch (gridDim.z = 2), from the plan's input kind and interlaced alone -- tile
// kernels only; launch_forward(), fill_jobs() and level1_kernel() read this and nothing else.  (Interlaced groups exist for YUY2 / 2vuy only: yuv422_input_served.)
FwdL1 GopBatch::forward_route() const
{
	if (enc_packed16(plan_.pixel_kind)) return FwdL1::GopPacked16;
	return plan_.interlaced ? FwdL1::FrameYuv422 : FwdL1::Yuv422;
}
const char *GopBatch::level1_kernel() const { return decode_ ? "" : kFwdL1Name[(int)forward_route()]; }

// The last level of a group's two frames: the intra path's kernel of the output (InvL1, one launch over both frames), then -- outputs made from 16-bit rows --
// the conversion of both frames' YU64 rows.
struct GopRoute { InvL1 l1; OutputRoute out; };

// What the output needs is output_route()'s answer for a 4:2:2 sample; here the family becomes the tile / row kernel the group launches (no strips, no block lists).
GopRoute GopBatch::route() const
{
	const OutputRoute o = output_route(ENC_YUV422, out_kind_, half_, plan_.interlaced);
	if (o.refusal) return { InvL1::Refused, o };
	switch (o.jobs) {
	case OutJobs::HalfYuv: return { half_yuv_kernel(o), o };
	case OutJobs::Planes16: return { plan_.interlaced ? InvL1::Refused : InvL1::Packed16, o };      // (YU64, v210 and RG24 of interlaced groups are refused at the C ABI)
	case OutJobs::Yuv: {
		if (o.convert != OutConvert::Rgb16) return { dec_rgb8(o.work) ? InvL1::Yuv422Rgb32 : (plan_.interlaced ? InvL1::FrameYuv422 : InvL1::Yuv422), o };
		// (the scratch rows are 16-byte aligned: 4 * width bytes, the width a multiple of 16: build_gop_plan)
		const int pitch[3] = { plan_.ch[0].w[0].pitch, plan_.ch[1].w[0].pitch, plan_.ch[2].w[0].pitch };
		return { frame_quads_fit(shape_override("CFHD_AMD_INVERSE"), plan_.ch[0].w[0].width, pitch) ? InvL1::FrameRows16 : InvL1::FrameRows16Col, o };
	}
	case OutJobs::HalfPacked: break;                     // (no output of a 4:2:2 sample)
	}
	return { InvL1::Refused, o };
}

GopBatch::GopBatch() {}
GopBatch::~GopBatch() { release(); }

void GopBatch::release()
{
	(void)hipSetDevice(device_);
	if (stream_) hipStreamSynchronize((hipStream_t)stream_);
	ent_ready_ = false;                              // (its buffers go with the object or with the next prepare_group(); it is not used before prepare_entropy() ran again)
	if (dec_ready_) { dec_.release(); dec_ready_ = false; }
	if (bdec_ready_) { bdec_.release(); bdec_ready_ = false; }
	for (void *&e : ev_) if (e) { (void)hipEventDestroy((hipEvent_t)e); e = nullptr; }
	collect_.release();
	launched_ = false;
	if (d_frames_) hipFree(d_frames_);
	if (h_frames_) hipHostFree(h_frames_);
	if (d_tmp_) hipFree(d_tmp_);
	if (d_coeff_) hipFree(d_coeff_);
	if (h_coeff_) hipHostFree(h_coeff_);
	if (d_jobs_) hipFree(d_jobs_);
	if (h_jobs_) hipHostFree(h_jobs_);
	if (stream_) device_stream_destroy(stream_);
	d_frames_ = h_frames_ = d_tmp_ = nullptr; d_coeff_ = h_coeff_ = nullptr; d_jobs_ = h_jobs_ = nullptr; stream_ = nullptr;
}

int GopBatch::prepare(const GopPlan &plan, bool decode, int out_pixel_kind, bool half, int ngroups)
{
	int rc = device_init();
	if (rc) return rc;
	release();
	// the job index of every launch stays in blockIdx.y / z: 6 n plane jobs (k_fwd_plane / k_inv_plane, k_dec_lowpass), 6 n planes of the packed-16 last level
	if (ngroups < 1 || 6 * (long long)ngroups > kMaxGridYZ) { g_err = "two-frame groups: the batch's job index would pass the grid limit"; return -2; }
	device_ = device_current(); (void)hipSetDevice(device_);
	plan_ = plan; decode_ = decode; out_kind_ = out_pixel_kind; half_ = decode && half; n_ = ngroups;
	group_plans_.clear(); group_dirty_.clear();
	const size_t nf = 2 * (size_t)n_;
	const GopRoute r = route();
	if (decode && r.l1 == InvL1::Refused) { g_err = "two-frame groups: output not served"; return -2; }
	HIPCHK((hipError_t)device_stream_create(&stream_));
	const int out_width = half_ ? plan.width / 2 : plan.width;      // (the output's own row size and row count, which may be half size)
	pitch_ = packed_frame_pitch(decode ? out_pixel_kind : plan.pixel_kind, out_width); rows_ = half_ ? plan.display_height / 2 : plan.display_height;
	frame_bytes_ = (size_t)pitch_ * rows_;
	if (!decode && plan.pixel_kind == PIX_AV28) frame_bytes_ = av28_frame_bytes(plan.width, plan.height, plan.display_height);      // one block, its pitch ignored (upload_frame)
	HIPCHK(hipMalloc((void **)&d_frames_, nf * frame_bytes_));
	HIPCHK(hipHostMalloc((void **)&h_frames_, nf * frame_bytes_, hipHostMallocPortable));
	if (decode && out_pixel_kind == PIX_V210) HIPCHK(hipMemsetAsync(d_frames_, 0, nf * frame_bytes_, (hipStream_t)stream_));      // (row padding beyond the last whole group of 48 pixels stays zero)
	tmp_pitch_ = 0; tmp_frame_bytes_ = 0;
	if (decode && r.out.convert != OutConvert::None) {
		tmp_pitch_ = packed_frame_pitch(PIX_YU64, out_width); tmp_frame_bytes_ = (size_t)tmp_pitch_ * rows_;
		HIPCHK(hipMalloc((void **)&d_tmp_, nf * tmp_frame_bytes_));
	}
	HIPCHK(hipMalloc((void **)&d_coeff_, (size_t)n_ * plan.coeff_elems * 2));
	HIPCHK(hipMemsetAsync(d_coeff_, 0, (size_t)n_ * plan.coeff_elems * 2, (hipStream_t)stream_));      // pad columns stay zero forever
	// (the host's copy of the pyramid serves the host coder of the C ABI's single group: a batch of groups never brings its pyramids to the host)
	HIPCHK(hipHostMalloc((void **)&h_coeff_, plan.coeff_elems * 2, hipHostMallocPortable));
	memset(h_coeff_, 0, plan.coeff_elems * 2);
	jobs_bytes_ = gop_jobs_bytes(n_);
	HIPCHK(hipMalloc(&d_jobs_, jobs_bytes_));
	HIPCHK(hipHostMalloc(&h_jobs_, jobs_bytes_, hipHostMallocPortable));
	memset(h_jobs_, 0, jobs_bytes_);
	fill_jobs();
	return 0;
}

void GopBatch::set_color_matrix(int m)
{
	if (m == matrix_) return;
	if (stream_) (void)hipStreamSynchronize((hipStream_t)stream_);
	matrix_ = m;
	if (h_jobs_) fill_jobs();
}

void GopBatch::set_plan(const GopPlan &plan)
{
	if (stream_) (void)hipStreamSynchronize((hipStream_t)stream_);
	plan_ = plan; group_plans_.clear();
	if (ent_ready_) ent_.set_group_plan(plan);
	fill_jobs();
}

int GopBatch::prepare_entropy(size_t sample_cap)
{
	(void)hipSetDevice(device_);
	ent_ready_ = false;
	if (decode_ || !d_coeff_) return -1;
	const int rc = ent_.prepare_group(plan_, n_, d_coeff_, plan_.coeff_elems, sample_cap, stream_);
	ent_ready_ = rc == 0;
	return rc;
}

int GopBatch::prepare_entropy_decode()
{
	(void)hipSetDevice(device_);
	bdec_ready_ = false;
	if (!decode_ || !d_coeff_) return -1;
	const int rc = bdec_.prepare(plan_, n_, d_coeff_, plan_.coeff_elems, out_kind_, stream_, device_);
	bdec_ready_ = rc == 0;
	return rc;
}

void GopBatch::set_timed(bool on)
{
	(void)hipSetDevice(device_);
	if (on) for (void *&e : ev_) if (!e && hipEventCreate((hipEvent_t *)&e) != hipSuccess) { (void)hipGetLastError(); e = nullptr; on = false; }
	timed_ = on;
}

float GopBatch::stage_ms(int k)
{
	float ms = 0;
	if (!timed_ || !launched_ || k < 0 || k > 2) return 0;
	// forward: events in launch order; inverse: the top wavelet runs first, the last level last
	const int a = decode_ ? 2 - k : k;
	if (hipEventElapsedTime(&ms, (hipEvent_t)ev_[a], (hipEvent_t)ev_[a + 1]) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return ms;
}

// (the names as a profiler shows them, "a+b": two launches in that order)
const char *GopBatch::stage_kernel(int k) const
{
	if (k < 0 || k > 2) return "";
	if (!decode_) {
		if (k == 0) return level1_kernel();
		if (k == 2) return "k_fwd_plane";
		return gop_temporal_lowpass_is_coded(plan_) ? "k_gop_temporal_fwd+k_fwd_plane+k_gop_quant_lowpass" : "k_gop_temporal_fwd+k_fwd_plane";
	}
	if (k == 2) return "k_inv_plane";
	if (k == 1) return "k_inv_plane+k_gop_temporal_inv";
	const GopRoute r = route();
	static const char *const conv[] = {"", "+k_yu64_to_v210", "+k_yu64_to_rgb24", "+k_yu64_to_rgb16", "+k_bayer_to_byr4"};
	snprintf(stage_name_[0], sizeof(stage_name_[0]), "%s%s", kInvL1Name[(int)r.l1], conv[(int)r.out.convert]);
	return stage_name_[0];
}

int GopBatch::launch_entropy_decode(const uint8_t *sample, size_t size, const ParsedGroup &pg, size_t sample_cap)
{
	(void)hipSetDevice(device_);
	if (!decode_ || !d_coeff_) return -1;
	if (!dec_ready_) {
		if (dec_.prepare(plan_, d_coeff_, sample_cap, out_kind_, stream_, device_)) return -1;
		dec_ready_ = true;
	}
	return dec_.launch(sample, size, pg);
}

void GopBatch::fill_jobs()
{
	for (int g = 0; g < n_; g++) fill_group_jobs(g);
	jobs_dirty_ = true;
}

// group g: its rows of the table, its pyramid, its two frames, its divisors
void GopBatch::fill_group_jobs(int g)
{
	const GopPlan &plan = group_plan(g);
	const int mpq = plan.midpoint_prequant;
	const OutputRoute o = decode_ ? route().out : OutputRoute();
	GopJobs j = gop_jobs_at(h_jobs_, n_);
	j.yuv += 2 * g; j.temp += 3 * g; j.mid += 6 * g; j.top += 3 * g; j.itop += 3 * g; j.imid += 6 * g; j.iyuv += 2 * g; j.l1 += 6 * g; j.half += 2 * g; j.fl1 += 6 * g; j.tq += 3 * g;
	int16_t *base = d_coeff_ + (size_t)g * plan.coeff_elems;
	for (int f = 0; f < 2; f++) {
		const int fi = 2 * g + f;                          // the frame's place in the batch: its buffers, its dither
		const uint8_t *frame = d_frames_ + frame_bytes_ * fi;
		const Level1 l1 = level1_of(plan, f, base);
		fill_fwd_yuv_job(j.yuv[f], frame, pitch_, plan.width, plan.height, plan.display_height, plan.pixel_kind, plan.precision, l1, mpq, plan.interlaced);
		if (!decode_ && forward_route() == FwdL1::GopPacked16)
			for (int c = 0; c < 3; c++) {                  // the intra path's loader of this input (EncodeBatch::fill_jobs), the bands and quantizers of the group's w[f]
				dev::FwdPlaneJob &p = j.fl1[3 * f + c];
				fill_fwd_plane_job(p, nullptr, 0, plan.ch[c].width, plan.ch[c].height, plan.ch[c].w[f].prescale, fwd_bands(l1, c), mpq);
				fill_packed16_loader(p, frame, pitch_, plan.pixel_kind, ENC_YUV422, plan.color_matrix, plan.width, plan.height, plan.precision, plan.display_height, 3, c);
			}
		if (!decode_) continue;
		// the last level of frame f: the intra path's job of the output's family (DecodeBatch::prepare) on the group's w[f].  Outputs made from 16-bit rows: the YU64
		// rows of frame f go to the scratch frame
		uint8_t *out = d_tmp_ ? d_tmp_ + tmp_frame_bytes_ * fi : d_frames_ + frame_bytes_ * fi;
		const int out_pitch = d_tmp_ ? tmp_pitch_ : pitch_;
		// (the matrix of frame 1 is the default one: the P-frame sample that hands it out carries no colour space tag, and the reference converts it with 709 -- pinned)
		const int matrix = f == 0 ? matrix_ : 0;
		switch (o.jobs) {
		case OutJobs::HalfYuv: fill_half_yuv_job(j.half[f], l1, o, rows_, matrix, out, out_pitch); break;
		case OutJobs::Planes16: fill_planes16_jobs(&j.l1[3 * f], l1, o, 3, 3, plan.precision, plan.display_height, fi, out, out_pitch); break;
		case OutJobs::Yuv: fill_inv_yuv_job(j.iyuv[f], l1, o, plan.precision, plan.display_height, matrix, fi, out, out_pitch); break;
		case OutJobs::HalfPacked: break;                 // (no output of a 4:2:2 sample)
		}
	}
	auto fwd = [&](dev::FwdPlaneJob &p, const int16_t *in, const GopWavelet &src, const GopWavelet &dst) { fill_fwd_plane_job(p, in, src.pitch, src.width, src.height, dst.prescale, fwd_bands(base, dst), mpq); };
	auto inv = [&](dev::InvPlaneJob &p, const GopWavelet &src, int16_t *out, int out_pitch) {
		memset(&p, 0, sizeof(p));
		for (int b = 0; b < 4; b++) p.band[b] = base + src.offset[b];
		p.band_pitch = src.pitch; p.width = src.width; p.height = src.height; p.descale = src.prescale;
		p.out = out; p.out_pitch = out_pitch; p.xstride = 1; p.precision = 0; p.display_height = 2 * src.height;
		// the unprescaled wavelets of a group (w[5] and w[3]) go through the reference's InvertSpatialQuantOverflowProtected16s and inherit the defect of its last
		// row (InvPlaneJob::ll_bottom_row_high): the reference decoder's pictures are the parity bar.  CFHD_AMD_GOP_BOTTOM_ROWS=fixed: the filter as meant (+5 dB).
		static const bool fixed = [] { const char *e = getenv("CFHD_AMD_GOP_BOTTOM_ROWS"); return e && strcmp(e, "fixed") == 0; }();
		p.ll_bottom_row_high = (src.prescale == 0 && !fixed) ? 1 : 0;
	};
	for (int c = 0; c < 3; c++) {
		const GopChannel &ch = plan.ch[c];
		dev::GopTemporalJob &t = j.temp[c];
		t.pitch = ch.w[2].pitch; t.height = ch.w[2].height; t.width = ch.w[2].width;
		if (!decode_) { t.a = base + ch.w[0].offset[0]; t.b = base + ch.w[1].offset[0]; t.x = base + ch.w[2].offset[0]; t.y = base + ch.w[2].offset[1]; }
		else { t.a = base + ch.w[2].offset[0]; t.b = base + ch.w[2].offset[1]; t.x = base + ch.w[0].offset[0]; t.y = base + ch.w[1].offset[0]; }
		fwd(j.mid[2 * c], base + ch.w[2].offset[1], ch.w[2], ch.w[3]);      // the temporal highpass band
		{                                                                    // ... whose lowpass band is divided behind the transform where the source asks for it
			const GopWavelet &w3 = ch.w[3];
			j.mid[2 * c].q[0] = make_q(1, mpq);
			j.tq[c].band = base + w3.offset[0]; j.tq[c].pairs = w3.pitch * w3.height / 2;
			j.tq[c].q.divisor = w3.quant[0]; j.tq[c].q.mid = 0; j.tq[c].q.mult = w3.quant[0] > 1 ? ((1u << 16) / (unsigned)w3.quant[0]) & 0xffffu : 0;
		}
		fwd(j.mid[2 * c + 1], base + ch.w[2].offset[0], ch.w[2], ch.w[4]);  // the temporal lowpass band
		fwd(j.top[c], base + ch.w[4].offset[0], ch.w[4], ch.w[5]);
		inv(j.itop[c], ch.w[5], base + ch.w[4].offset[0], ch.w[4].pitch);
		inv(j.imid[2 * c], ch.w[4], base + ch.w[2].offset[0], ch.w[2].pitch);
		inv(j.imid[2 * c + 1], ch.w[3], base + ch.w[2].offset[1], ch.w[2].pitch);
	}
}

int GopBatch::set_group_plan(int g, const GopPlan &plan)
{
	if (g < 0 || g >= n_ || decode_ || !h_jobs_ || plan.coeff_elems != plan_.coeff_elems || plan.interlaced != plan_.interlaced || plan.pixel_kind != plan_.pixel_kind) return -1;
	if (group_plans_.empty()) group_plans_.assign((size_t)n_, plan_);
	if (group_dirty_.empty()) group_dirty_.assign((size_t)n_, 0);
	group_plans_[(size_t)g] = plan;
	fill_group_jobs(g);
	group_dirty_[(size_t)g] = 1;
	return 0;
}

// The encoder's rows that carry divisors: level 1 of both frames (either job family), the temporal highpass wavelet with the division of its lowpass band, the two
// wavelets above.  Runs of rewritten groups travel in one copy per table.
int GopBatch::sync_jobs()
{
	hipStream_t st = (hipStream_t)stream_;
	if (jobs_dirty_) {
		HIPCHK(hipMemcpyAsync(d_jobs_, h_jobs_, jobs_bytes_, hipMemcpyHostToDevice, st));
		jobs_dirty_ = false; group_dirty_.assign(group_dirty_.size(), 0);
		return 0;
	}
	const GopJobs h = gop_jobs_at(h_jobs_, n_), d = gop_jobs_at(d_jobs_, n_);
	for (int g = 0; g < (int)group_dirty_.size();) {
		if (!group_dirty_[(size_t)g]) { g++; continue; }
		int e = g;
		while (e < (int)group_dirty_.size() && group_dirty_[(size_t)e]) group_dirty_[(size_t)e++] = 0;
		const size_t k = (size_t)(e - g);
		HIPCHK(hipMemcpyAsync(d.yuv + 2 * g, h.yuv + 2 * g, 2 * k * sizeof(dev::FwdYuvJob), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d.fl1 + 6 * g, h.fl1 + 6 * g, 6 * k * sizeof(dev::FwdPlaneJob), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d.mid + 6 * g, h.mid + 6 * g, 6 * k * sizeof(dev::FwdPlaneJob), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d.top + 3 * g, h.top + 3 * g, 3 * k * sizeof(dev::FwdPlaneJob), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(d.tq + 3 * g, h.tq + 3 * g, 3 * k * sizeof(dev::GopQuantJob), hipMemcpyHostToDevice, st));
		g = e;
	}
	return 0;
}

int GopBatch::upload_frame(int f, const void *frame, int pitch)
{
	(void)hipSetDevice(device_);
	if (decode_ || f < 0 || f >= 2 * n_) return -1;
	const uint8_t *src = (const uint8_t *)frame;
	const bool av28 = plan_.pixel_kind == PIX_AV28;      // two planes walked as tightly packed rows whatever the pitch; its sign still moves the start (EncodeBatch::upload_frame)
	if (pitch < 0) { src += (ptrdiff_t)(rows_ - 1) * pitch; pitch = -pitch; }     // encoder.c:1957
	uint8_t *dst = h_frames_ + frame_bytes_ * f;
	if (pitch == pitch_ || av28) memcpy(dst, src, frame_bytes_);
	else for (int r = 0; r < rows_; r++) memcpy(dst + (size_t)r * pitch_, src + (size_t)r * pitch, (size_t)pitch_);
	HIPCHK(hipMemcpyAsync(d_frames_ + frame_bytes_ * f, dst, frame_bytes_, hipMemcpyHostToDevice, (hipStream_t)stream_));
	return 0;
}

// upload_frame for a frame that lies in HBM on the batch's device (EncodeBatch::upload_frame_device): one strided device-to-device copy on the batch's stream.
int GopBatch::upload_frame_device(int f, const void *d_frame, int pitch)
{
	(void)hipSetDevice(device_);
	if (decode_ || f < 0 || f >= 2 * n_ || !d_frame) return -1;
	const uint8_t *src = (const uint8_t *)d_frame;
	if (pitch < 0) { src += (ptrdiff_t)(rows_ - 1) * pitch; pitch = -pitch; }     // encoder.c:1957
	if (plan_.pixel_kind == PIX_AV28) {                     // (one block of two planes, walked as tightly packed rows whatever the pitch: upload_frame)
		HIPCHK(hipMemcpyAsync(d_frames_ + frame_bytes_ * f, src, frame_bytes_, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
		return 0;
	}
	if (pitch < pitch_) return -1;
	HIPCHK(hipMemcpy2DAsync(d_frames_ + frame_bytes_ * f, (size_t)pitch_, src, (size_t)pitch, (size_t)pitch_, (size_t)rows_, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
	return 0;
}

int GopBatch::upload_frames_device_planar(int first, int count, const void *d_frames, size_t frame_stride, int row_pitch, int layout)
{
	(void)hipSetDevice(device_);
	if (decode_) return -1;
	return collect_planar_frames(plan_.pixel_kind, d_frames_, frame_bytes_, pitch_, plan_.width, rows_, 2 * n_, first, count, d_frames, frame_stride, row_pitch, layout, stream_, collect_);
}

// Frame f as the encoder's batch holds it, packed: rows_ rows of pitch_ bytes (av28: the frame's one block), behind whatever the stream holds.
int GopBatch::download_input_frame(int f, void *out, int pitch)
{
	(void)hipSetDevice(device_);
	const size_t row = pitch_ ? (size_t)pitch_ : frame_bytes_, nrows = pitch_ ? (size_t)rows_ : 1;
	if (decode_ || f < 0 || f >= 2 * n_ || !out || pitch < 0 || (size_t)pitch < row) return -1;
	HIPCHK(hipMemcpy2DAsync(out, (size_t)pitch, d_frames_ + frame_bytes_ * f, row, row, nrows, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
	return 0;
}

// All 2 n frames from the caller's memory, queued on the batch's stream: one copy as they are when they lie back to back at the batch's own pitch in a registered
// buffer, otherwise staged through the batch's pinned frames by the calling thread (the caller waits for the previous pass before it submits the next: the staging
// buffer is free) and copied in one piece.
int GopBatch::upload_frames(const void *frames, size_t frame_stride, int pitch)
{
	(void)hipSetDevice(device_);
	if (decode_ || !frames || pitch <= 0) return -1;
	const size_t total = 2 * (size_t)n_ * frame_bytes_;
	const bool av28 = plan_.pixel_kind == PIX_AV28;
	if ((pitch == pitch_ || av28) && frame_stride == frame_bytes_ && host_buffer_is_registered(frames, total)) {
		HIPCHK(hipMemcpyAsync(d_frames_, frames, total, hipMemcpyHostToDevice, (hipStream_t)stream_));
		return 0;
	}
	for (int f = 0; f < 2 * n_; f++) {
		const uint8_t *src = (const uint8_t *)frames + frame_stride * (size_t)f;
		uint8_t *dst = h_frames_ + frame_bytes_ * f;
		if (pitch == pitch_ || av28) memcpy(dst, src, frame_bytes_);
		else for (int r = 0; r < rows_; r++) memcpy(dst + (size_t)r * pitch_, src + (size_t)r * pitch, (size_t)(pitch < pitch_ ? pitch : pitch_));
	}
	HIPCHK(hipMemcpyAsync(d_frames_, h_frames_, total, hipMemcpyHostToDevice, (hipStream_t)stream_));
	return 0;
}

int GopBatch::launch_forward(int first, int count)
{
	if (first < 0 || count < 1 || first + count > n_) return -1;
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	const int rcj = sync_jobs();
	if (rcj) return rcj;
	GopJobs j = gop_jobs_at(d_jobs_, n_);
	// (a window: every table from its first group's rows on -- the jobs hold the addresses of their own frames and pyramids)
	j.yuv += 2 * first; j.fl1 += 6 * first; j.temp += 3 * first; j.mid += 6 * first; j.top += 3 * first; j.tq += 3 * first;
	(void)hipGetLastError();
	if (timed_) HIPCHK(hipEventRecord((hipEvent_t)ev_[0], st));
	// level 1 of all frames (grid z = 2 count) through the intra path's launcher: the spatial transform, or -- interlaced groups -- the frame transform of interlaced intra
	// frames (the two kernels share the job table), or -- the 10-bit, 16-bit and RGB inputs -- the packed-16 loaders, the planes of a tile row side by side in gridDim.x
	const int luma_tiles = (plan_.ch[0].width / 2 + dev::TW - 1) / dev::TW, chroma_tiles = (plan_.ch[1].width / 2 + dev::TW - 1) / dev::TW;
	const int rc = launch_first_level(forward_route(), { plan_.width, plan_.height, 2 * count, j.yuv, j.fl1, nullptr, 3, plan_.pixel_kind, luma_tiles, chroma_tiles }, st);
	if (rc) return rc;
	if (timed_) HIPCHK(hipEventRecord((hipEvent_t)ev_[1], st));
	const GopWavelet &t = plan_.ch[0].w[2];
	dev::k_gop_temporal_fwd<<<dim3((unsigned)((t.pitch * t.height / 2 + dev::NTHREADS - 1) / dev::NTHREADS), 3 * count), dev::NTHREADS, 0, st>>>(j.temp);
	launch_fwd_plane_tiles(j.mid, t.width, t.height, 6 * count, st);
	if (!decode_ && gop_temporal_lowpass_is_coded(plan_)) {
		const GopWavelet &w3 = plan_.ch[0].w[3];                         // (luma is the largest of the three bands)
		dev::k_gop_quant_lowpass<<<dim3((unsigned)((w3.pitch * w3.height / 2 + dev::NTHREADS - 1) / dev::NTHREADS), 3 * count), dev::NTHREADS, 0, st>>>(j.tq);
	}
	if (timed_) HIPCHK(hipEventRecord((hipEvent_t)ev_[2], st));
	const GopWavelet &m = plan_.ch[0].w[4];
	launch_fwd_plane_tiles(j.top, m.width, m.height, 3 * count, st);
	HIPCHK(hipGetLastError());
	if (timed_) { HIPCHK(hipEventRecord((hipEvent_t)ev_[3], st)); launched_ = true; }
	return 0;
}

int GopBatch::download_coeffs()
{
	(void)hipSetDevice(device_);
	HIPCHK(hipMemcpyAsync(h_coeff_, d_coeff_, plan_.coeff_elems * 2, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	return 0;
}

int GopBatch::launch_inverse(uint32_t dither_seed, bool coeffs_on_device)
{
	(void)hipSetDevice(device_);
	hipStream_t st = (hipStream_t)stream_;
	if (jobs_dirty_) { HIPCHK(hipMemcpyAsync(d_jobs_, h_jobs_, jobs_bytes_, hipMemcpyHostToDevice, st)); jobs_dirty_ = false; }
	if (!coeffs_on_device) HIPCHK(hipMemcpyAsync(d_coeff_, h_coeff_, plan_.coeff_elems * 2, hipMemcpyHostToDevice, st));
	if (!coeffs_on_device && n_ != 1) return -1;          // (the host's pyramid is the single group's)
	GopJobs j = gop_jobs_at(d_jobs_, n_);
	const int ng = active_groups();                      // (the tables hold every group's rows; a short pass launches the first ones)
	(void)hipGetLastError();
	if (timed_) HIPCHK(hipEventRecord((hipEvent_t)ev_[0], st));
	const GopWavelet &top = plan_.ch[0].w[5], &mid = plan_.ch[0].w[4], &t = plan_.ch[0].w[2], &l1 = plan_.ch[0].w[0];
	dev::k_inv_plane<<<dim3((top.width + dev::ITW - 1) / dev::ITW, (top.height + dev::ITH - 1) / dev::ITH, 3 * ng), dev::NTHREADS, 0, st>>>(j.itop);
	if (timed_) HIPCHK(hipEventRecord((hipEvent_t)ev_[1], st));
	dev::k_inv_plane<<<dim3((mid.width + dev::ITW - 1) / dev::ITW, (mid.height + dev::ITH - 1) / dev::ITH, 6 * ng), dev::NTHREADS, 0, st>>>(j.imid);
	dev::k_gop_temporal_inv<<<dim3((unsigned)((t.pitch * t.height / 2 + dev::NTHREADS - 1) / dev::NTHREADS), 3 * ng), dev::NTHREADS, 0, st>>>(j.temp);
	if (timed_) HIPCHK(hipEventRecord((hipEvent_t)ev_[2], st));
	// the last level of all frames (grid z = 2 n): the intra path's kernels through the intra path's launcher
	const GopRoute r = route();
	const int rc = launch_last_level(r.l1, { l1.width, l1.height, rows_, 2 * ng, plan_.interlaced, j.iyuv, j.l1, j.half, nullptr, 3, dec_words_per_position(PIX_YU64, 3) }, dither_seed, st);
	if (rc) return rc;
	// the conversion runs over all frames in one launch -- two when the frames 0 take another matrix than the frames 1 (fill_jobs; v210 takes none): the first frames
	// of all groups, then the second ones, each launch striding over two frames; a frame 1 then runs as z = g with the seed that gives the single group's the dither of z = 1
	auto convert = [&](int f, int nf, size_t step, int m) {
		launch_convert(r.out, d_tmp_ + tmp_frame_bytes_ * f, tmp_pitch_, tmp_frame_bytes_ * step, d_frames_ + frame_bytes_ * f, pitch_, frame_bytes_ * step, half_ ? plan_.width / 2 : plan_.width, rows_, 0, nf, m,
		               dither_seed + 0x9E3779B9u * (uint32_t)f, nullptr, st);
	};
	if (matrix_ == 0 || r.out.convert == OutConvert::V210) convert(0, 2 * ng, 1, 0); else { convert(0, ng, 2, matrix_); convert(1, ng, 2, 0); }
	HIPCHK(hipGetLastError());
	if (timed_) { HIPCHK(hipEventRecord((hipEvent_t)ev_[3], st)); launched_ = true; }
	return 0;
}

int GopBatch::download_frame(int f, void *, int)
{
	(void)hipSetDevice(device_);
	if (!decode_ || f < 0 || f >= 2 * n_) return -1;
	HIPCHK(hipMemcpyAsync(h_frames_ + frame_bytes_ * f, d_frames_ + frame_bytes_ * f, frame_bytes_, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	return 0;
}

// All 2 n pictures on their way to the host behind the inverse transform: one copy into the batch's pinned frames; finish_frame() hands each to the caller behind wait().
int GopBatch::download_frames(void *out, size_t, int pitch)
{
	(void)hipSetDevice(device_);
	if (!decode_ || !out || pitch <= 0) return -1;
	HIPCHK(hipMemcpyAsync(h_frames_, d_frames_, 2 * (size_t)active_groups() * frame_bytes_, hipMemcpyDeviceToHost, (hipStream_t)stream_));
	return 0;
}

int GopBatch::finish_frame(int f, void *out, int pitch)
{
	if (!decode_ || f < 0 || f >= 2 * n_) return -1;
	const uint8_t *src = h_frames_ + frame_bytes_ * f;
	if (pitch == pitch_) memcpy(out, src, frame_bytes_);
	else for (int r = 0; r < rows_; r++) memcpy((uint8_t *)out + (ptrdiff_t)r * pitch, src + (size_t)r * pitch_, (size_t)pitch_);
	return 0;
}

int GopBatch::wait()
{
	(void)hipSetDevice(device_);
	HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
	collect_.resolve();
	return 0;
}

} // namespace cfhd
