// cfhd_api_decoder.inc -- part of cfhd_api.cpp (one translation unit: the parts are #included there in this order, they share the handle types of an unnamed namespace).
// CFHD_OpenDecoder ... CFHD_CloseDecoder, thumbnails, sample header (Common/CFHDDecoder.h:203-310; DecoderSDK/CFHDDecoder.cpp, SampleDecoder.cpp).

// =============================================================================================
// Decoder
// =============================================================================================
CFHD_Error CFHD_OpenDecoder(CFHD_DecoderRef *out, CFHD_ALLOCATOR *)
{
	if (!out) return ERR_INVALID_ARGUMENT;
	*out = new (std::nothrow) Decoder;
	// a process that owns several GPUs deals its decoder handles over them round robin (one process per GPU keeps them on its own)
	static std::atomic<int> handles{0};
	if (*out) ((Decoder *)*out)->device = device_of_unit(handles.fetch_add(1));
	return *out ? ERR_OKAY : ERR_OUTOFMEMORY;
}

// The output formats this decoder offers for the given sample (all of them without one): what CFHD_PrepareToDecode accepts for its encoded format.
CFHD_Error CFHD_GetOutputFormats(CFHD_DecoderRef ref, void *sample, size_t size, CFHD_PixelFormat *arr, int len, int *count)
{
	if (!ref || !arr) return ERR_INVALID_ARGUMENT;
	ParsedSample ps;
	const bool known = sample && parse_sample((const uint8_t *)sample, size, &ps) >= 0;
	uint32_t fmts[32]; int total = 0;
	auto add = [&](uint32_t f) { for (int i = 0; i < total; i++) if (fmts[i] == f) return; fmts[total++] = f; };      // (without a sample: every format once)
	if (!known || ps.encoded_format == ENC_YUV422) { add(FMT_YUY2); add(FMT_2VUY); add(FMT_YU64); add(FMT_V210); add(FMT_RG24); }
	if (!known || ps.encoded_format == ENC_RGB444) { add(FMT_RG48); add(FMT_RG24); add(FMT_BGRA); add(FMT_BGRa); add(FMT_R210); add(FMT_DPX0); add(FMT_AB10); add(FMT_AR10); add(FMT_RG30); add(FMT_B64A); }
	if (!known || ps.encoded_format == ENC_RGBA4444) { add(FMT_B64A); add(FMT_BGRA); add(FMT_BGRa); add(FMT_RG48); }
	if (!known || ps.encoded_format == ENC_BAYER) add(FMT_BYR4);
	int n = 0;
	for (; n < total && n < len; n++) arr[n] = fmts[n];
	if (count) *count = n;
	return ERR_OKAY;
}

CFHD_Error CFHD_GetSampleInfo(CFHD_DecoderRef ref, void *sample, size_t size, CFHD_SampleInfoTag tag, void *value, size_t buffer_size)
{
	if (!ref || !sample || !value || buffer_size < 4) return ERR_INVALID_ARGUMENT;
	ParsedSample ps;
	if (parse_sample((const uint8_t *)sample, size, &ps) < 0) return ERR_BADSAMPLE;
	int32_t v = 0;
	switch (tag) {
	case 0: v = 1; break;                                 // CFHD_SAMPLE_INFO_CHANNELS (video channels: 2D)
	case 1: v = ps.encoded_format == ENC_BAYER ? 2 * ps.width : ps.width; break;   // CFHD_SAMPLE_DISPLAY_WIDTH (Bayer samples carry the component plane size, decoder.c:2617)
	case 2: v = 0; break;                                 // CFHD_SAMPLE_DISPLAY_HEIGHT: the reference answers 0 for every sample (its parser keeps the tag in a local, decoder.c:2156, and SAMPLE_HEADER::display_height stays cleared); callers take the height from CFHD_PrepareToDecode
	case 3: v = 1; break;                                 // CFHD_SAMPLE_KEY_FRAME (intra only)
	case 4: v = ps.progressive; break;                    // CFHD_SAMPLE_PROGRESSIVE
	// CFHD_SAMPLE_ENCODED_FORMAT: the public CFHD_EncodedFormat enum (YUV_422 0, RGB_444 1, RGBA_4444 2, BAYER 3), not the bitstream's
	// ENCODED_FORMAT code (SampleDecoder.cpp:821-840)
	case 5: v = ps.encoded_format == ENC_RGB444 ? 1 : (ps.encoded_format == ENC_RGBA4444 ? 2 : (ps.encoded_format == ENC_BAYER ? 3 : 0)); break;
	case 6: v = (10 << 16) | (1 << 8) | 0; break;         // CFHD_SAMPLE_SDK_VERSION
	case 7: v = ((ps.version >> 12) << 16) | (((ps.version >> 8) & 0xf) << 8) | (ps.version & 0xff); break;   // CFHD_SAMPLE_ENCODE_VERSION
	default: return ERR_INVALID_ARGUMENT;
	}
	memcpy(value, &v, 4);
	return ERR_OKAY;
}

// What a 4:2:2 sample `width` pixels wide decodes to -- intra samples and two-frame groups alike (CFHD_PrepareToDecode; the interlaced-only refusals follow at
// CFHD_DecodeSample, where the scan is known):
//   YUY2 / 2vuy: always;
//   YU64 (16-bit words Y0 C1 Y1 C2; the reference's planar 16-bit row route; half resolution: frame.c:11146 ConvertLowpass16sToYUV64, k_half_yu64): the tail-column
//     rule of the 16-bit rows is restated for chroma bands of 16 columns and more;
//   v210 (the YU64 words >> 6, three to a 32-bit word: k_yu64_to_v210; half resolution: frame.c:12139 ConvertLowpass16s10bitToV210 = the half-resolution YU64 words
//     >> 6): widths of whole six-pixel groups;
//   RG24 (the YU64 rows through the reference's scalar colour conversion with its 15-bit dither, k_yu64_to_rgb24; half resolution: frame.c:8504, k_half_rgb24);
//   BGRA / BGRa (the reference's fused horizontal pass + 8-bit colour conversion, spatial.c:29577: k_inv_yuv422_rgb32) and RG48 / b64a (its 16-bit rows +
//     RGB2YUV.c:1760: k_yu64_to_rgb16) -- the last four rows of TestCFHD's table; half resolution: the level-1 lowpass planes through frame.c:8504's RGB32 branch
//     -- its SSE2 loop, so half widths that are multiples of 16 -- and frame.c:9567 ConvertLowpass16sYUVtoRGB48: k_half_rgb24's other modes.
// Not the 10-bit RGB words, BYR4 or the encoder-only inputs.
static bool yuv422_output_served(int kind, int width, bool half)
{
	switch (kind) {
	case PIX_YUY2: case PIX_2VUY: return true;
	case PIX_YU64: case PIX_RG24: return width >= 128;
	case PIX_V210: return width >= 128 && (half ? width / 2 : width) % 6 == 0;
	case PIX_BGRA: case PIX_BGRa: return width >= 32 && (!half || (width / 2) % 16 == 0);
	case PIX_RG48: case PIX_B64A: return width >= (half ? 32 : 128);
	default: return false;
	}
}

static const char *const kUncompressedRefusal = "uncompressed sample (UNCOMPRESS chunk): the uncompressed mode is not built";

CFHD_Error CFHD_PrepareToDecode(CFHD_DecoderRef ref, int, int, CFHD_PixelFormat fmt, CFHD_DecodedResolution resolution, CFHD_DecodingFlags,
                                void *sample, size_t size, int *aw, int *ah, CFHD_PixelFormat *af)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref || !sample) return ERR_INVALID_ARGUMENT;
	Decoder *d = (Decoder *)ref;
	{
		// a stream of two-frame groups starts with a sequence header, or is entered at a group (or at the header of a group's second frame)
		const uint8_t *s8 = (const uint8_t *)sample;
		const int first_tag = size >= 4 ? (int16_t)((s8[0] << 8) | s8[1]) : 0, sample_type = size >= 4 ? ((s8[2] << 8) | s8[3]) : 0;
		ParsedGroup pg;
		const bool group_stream = first_tag == TAG_SAMPLE && (sample_type == 7 || sample_type == 2 || sample_type == 1);
		if (group_stream) {
			// (only the header tags matter here: the caller may pass the first 512 bytes of the sample)
			(void)parse_group_sample(s8, size < 160 ? size : 160, &pg);
			if (pg.width <= 0 || pg.height <= 0) return ERR_BADSAMPLE;
			// every output an intra 4:2:2 sample of this width decodes to, full and half resolution: each frame's level-1 wavelet goes through the intra route of the output
			if (resolution != 1 && resolution != 0 && resolution != 2) return ERR_BAD_RESOLUTION;
			const bool half = resolution == 2;
			const int kind = pixel_kind_of(fmt);
			if (!yuv422_output_served(kind, pg.width, half)) return ERR_BADFORMAT;
			const int display = pg.display_height ? pg.display_height : pg.height;
			if (!build_gop_plan(&d->gplan, pg.width, display, kind == PIX_2VUY ? PIX_2VUY : PIX_YUY2)) return ERR_BADFORMAT;      // (the plan's pixel kind is the encoder's input)
			d->gop = true; d->gop_ready = false; d->gop_second = false;
			d->out_format = fmt; d->out_kind = kind; d->half = half; d->prepared = true;
			d->plan = FramePlan(); d->plan.width = pg.width; d->plan.height = d->gplan.height; d->plan.display_height = display;
			if (aw) *aw = half ? pg.width / 2 : pg.width;
			if (ah) *ah = half ? display / 2 : display;
			if (af) *af = fmt;
			return ERR_OKAY;
		}
		d->gop = false;
	}
	if (parse_sample((const uint8_t *)sample, size, &d->header) < 0) return ERR_BADSAMPLE;
	// a sample of the reference's uncompressed mode (v210, 10-bit RGB and Bayer inputs with the uncompressed bits in the quality word): not built.  Refused here when the
	// bytes the caller passed reach the chunk tag, at CFHD_DecodeSample otherwise
	if (d->header.uncompressed) { device_set_last_error(kUncompressedRefusal); d->prepared = false; return ERR_BADFORMAT; }
	// CFHD_DECODED_RESOLUTION_FULL (1; 0 = unknown is taken as full) and _HALF (2): the level-1 lowpass planes shown as the picture
	// (decoder.c:14124, :26752).  Quarter / thumbnail resolutions are not built.
	if (resolution != 1 && resolution != 0 && resolution != 2) return ERR_BAD_RESOLUTION;
	const bool half = resolution == 2;
	const int encf = d->header.encoded_format;

	if ((encf != ENC_YUV422 && encf != ENC_RGB444 && encf != ENC_RGBA4444 && encf != ENC_BAYER) || d->header.transform_type != 0) return ERR_BADFORMAT;
	int kind = pixel_kind_of(fmt);
	if (kind == PIX_NONE) return ERR_BADFORMAT;
	// 4:2:2 samples decode to the packed 4:2:2 formats, YU64, v210 and the RGB outputs of yuv422_output_served (the same gate as two-frame groups)
	if (encf == ENC_YUV422) { if (!yuv422_output_served(kind, d->header.width, half)) return ERR_BADFORMAT; }
	else {
		// RGB 4:4:4 samples decode to RG48 (wavelet.c:4947), RGBA 4:4:4:4 samples to b64a (bayer.c:11916 Row16uFull2OutputFormat); colour conversions between the
		// families (ConvertLib / the colour part of the active-metadata pipeline in the reference) are not built; YU64 and v210 are 4:2:2 samples' only
		if (kind == PIX_YU64 || kind == PIX_V210) return ERR_BADFORMAT;
		// ... and RGB 4:4:4 samples to the 8-bit pixels RG24 / BGRA / BGRa (the RG48 reconstruction reduced with the reference's four-bit dither; full resolution)
		const bool rgb8 = kind == PIX_RG24 || kind == PIX_BGRA || kind == PIX_BGRa;
		// ... and RGBA 4:4:4:4 samples to BGRA / BGRa (no dither there: (12-bit component + 2) >> 4, the alpha expanded from that rounded value)
		const bool rgba8 = (kind == PIX_BGRA || kind == PIX_BGRa) && encf == ENC_RGBA4444;
		// (half resolution -- frame.c:7150 ConvertLowpassRGB444ToRGB -- for the outputs of RGB 4:4:4 samples: 8-bit, 10-bit, b64a; k_half_rgb)
		if (rgb8 && ((encf != ENC_RGB444 && !rgba8) || d->header.width < 32)) return ERR_BADFORMAT;
		// ... and to the 10-bit RGB words r210 / DPX0 / AB10 / AR10 ((value before the final >> 1, + 3) >> 3 per component: a model fitted on the reference
		// decoder and pinned word for word on the CPU, equal to the reference decoder on the GPU)
		const bool rgb10 = kind >= PIX_R210 && kind <= PIX_AR10;
		if (rgb10 && (encf != ENC_RGB444 || d->header.width < 32)) return ERR_BADFORMAT;
		// ... and Bayer samples to BYR4: the raw mosaic, no demosaic (the four planes as 16-bit rows, recombined per quad and sent through the reference's linear-restore
		// table: DecodeBatch / k_bayer_to_byr4; full resolution)
		const bool bayer_as_byr4 = kind == PIX_BYR4 && encf == ENC_BAYER && !half && d->header.width >= 32;
		if ((encf == ENC_BAYER) != bayer_as_byr4) return ERR_BADFORMAT;
		if ((kind == PIX_BYR4 && !bayer_as_byr4) || kind == PIX_BYR5 || kind == PIX_RG64 || (kind >= PIX_R210 && kind <= PIX_AR10 && !rgb10)) return ERR_BADFORMAT;     // encoder inputs only
		// ... and RGB 4:4:4 samples to b64a (the RG48 words behind a constant alpha word 0xfff0, full resolution: what TestCFHD's b64a -> RGB 4:4:4 row decodes to)
		const bool b64a_of_444 = kind == PIX_B64A && encf == ENC_RGB444;
		// ... and RGBA 4:4:4:4 samples to RG48 (the RG48 route on planes G, R, B, the alpha plane left behind; full and half resolution)
		const bool rg48_of_4444 = kind == PIX_RG48 && encf == ENC_RGBA4444;
		if ((encf == ENC_RGB444) != ((kind == PIX_RG48 && !rg48_of_4444) || (rgb8 && !rgba8) || rgb10 || b64a_of_444) ||
		    (encf == ENC_RGBA4444) != ((kind == PIX_B64A && !b64a_of_444) || rgba8 || rg48_of_4444)) return ERR_BADFORMAT;
	}
	bool ok;
	plan_from_sample(d->header, kind, &d->plan, &ok);
	if (!ok) return ERR_BADSAMPLE;
	d->out_format = fmt; d->out_kind = kind; d->prepared = true; d->batch_ready = false; d->half = half;
	d->service = nullptr;                                 // (looked up again for the new geometry by the next concurrent decode)
	const int quad = encf == ENC_BAYER ? 2 : 1;         // (Bayer samples carry the size of their component planes)
	if (aw) *aw = half ? d->header.width / 2 : quad * d->header.width;
	if (ah) *ah = half ? d->header.display_height / 2 : quad * d->header.display_height;
	if (af) *af = fmt;
	return ERR_OKAY;
}

static int pixel_size_of(uint32_t fmt)
{
	switch (fmt) {
	case FOURCC_BE('Y', 'U', 'Y', '2'): case FOURCC_BE('2', 'v', 'u', 'y'): case FOURCC_BE('y', 'u', 'y', 'v'):
	case FOURCC_BE('B', 'Y', 'R', '2'): case FOURCC_BE('B', 'Y', 'R', '4'): return 2;
	case FOURCC_BE('R', 'G', '2', '4'): return 3;
	case FOURCC_BE('B', 'G', 'R', 'A'): case FOURCC_BE('B', 'G', 'R', 'a'): case FOURCC_BE('r', '2', '1', '0'): case FOURCC_BE('D', 'P', 'X', '0'):
	case FOURCC_BE('R', 'G', '3', '0'): case FOURCC_BE('A', 'B', '1', '0'): case FOURCC_BE('A', 'R', '1', '0'): case FOURCC_BE('Y', 'U', '6', '4'): return 4;
	case FOURCC_BE('R', 'G', '4', '8'): case FOURCC_BE('W', 'P', '1', '3'): return 6;
	case FOURCC_BE('b', '6', '4', 'a'): case FOURCC_BE('R', 'G', '6', '4'): case FOURCC_BE('W', '1', '3', 'A'): return 8;
	default: return 0;
	}
}

CFHD_Error CFHD_GetPixelSize(CFHD_PixelFormat fmt, uint32_t *out)
{
	if (!out) return ERR_INVALID_ARGUMENT;
	*out = (uint32_t)pixel_size_of(fmt);
	return ERR_OKAY;
}

CFHD_Error CFHD_GetImagePitch(uint32_t width, CFHD_PixelFormat fmt, int32_t *out)
{
	if (!out) return ERR_INVALID_ARGUMENT;
	if (fmt == FMT_V210) { *out = (int32_t)((width + 47u) / 48u * 128u); return ERR_OKAY; }      // six pixels in 16 bytes, rows of whole 48-pixel groups (as the reference answers)
	*out = (int32_t)(((width * (uint32_t)pixel_size_of(fmt)) + 15u) & ~15u);              // SampleDecoder.cpp:290-305
	return ERR_OKAY;
}

CFHD_Error CFHD_GetImageSize(uint32_t width, uint32_t height, CFHD_PixelFormat fmt, CFHD_VideoSelect videoselect, CFHD_Stereo3DType stereotype, uint32_t *out)
{
	if (!out) return ERR_INVALID_ARGUMENT;
	int32_t pitch; CFHD_GetImagePitch(width, fmt, &pitch);
	uint32_t size = (uint32_t)pitch * height;
	if (stereotype == 0 && videoselect == 3) size *= 2;
	*out = size;
	return ERR_OKAY;
}

static CFHD_Error decode_on_handle(Decoder *d, const ParsedSample &ps, const uint8_t *s, size_t size, void *out, int32_t pitch, bool interlaced);

// Samples of a stream of two-frame groups (decoder.c:11180 DecodeSampleGroup, :11426 DecodeSampleFrame): the sequence header changes nothing, the
// group is decoded whole -- run-length / VLC stage on the host, the inverse transforms on the GPU (GopBatch) -- and gives its first frame, the
// P-frame sample behind it gives the second.
static CFHD_Error decode_group_sample(Decoder *d, const uint8_t *s, size_t size, void *out, int32_t pitch)
{
	const GopPlan &gp = d->gplan;
	auto fail_zero = [&](int err) {                                       // (the output's own row size and row count: half size at half resolution)
		const int rowbytes = packed_frame_pitch(d->out_kind, d->half ? gp.width / 2 : gp.width), rows = d->half ? gp.display_height / 2 : gp.display_height;
		for (int r = 0; r < rows; r++) memset((uint8_t *)out + (ptrdiff_t)r * pitch, 0, (size_t)rowbytes);
		return err;
	};
	ParsedGroup pg;
	const int rc = parse_group_sample(s, size, &pg);
	if (rc < 0) return fail_zero(ERR_BADSAMPLE);
	if (pg.sample_type == 7) return ERR_OKAY;                            // sequence header: no picture (the reference leaves the buffer alone too)
	if (pg.sample_type == 1) {                                           // the second frame of the last group
		if (!d->gop_second) return fail_zero(ERR_BADSAMPLE);
		d->gop_batch.finish_frame(1, out, pitch);
		d->gop_second = false;
		return ERR_OKAY;
	}
	if (pg.sample_type != 2 || pg.width != gp.width || pg.height != gp.height || pg.precision != 10) return fail_zero(ERR_BADSAMPLE);
	// Groups of interlaced frames (YUV_INTERLACED | 2FRAME_GOP) carry no SAMPLE_FLAGS tag (decoder.c:13397 sets `progressive` only from the tag): frame transform at
	// level 1 of both frames, the band 2 of both frame wavelets difference coded in code set 18 (subbands 12 and 15) -- and nowhere else
	const bool interlaced = !pg.progressive;
	for (int c = 0; c < 3; c++) for (int k = 0; k < kGopWavelets; k++) for (int b = 0; b < 4; b++)
		if (pg.band[c][k][b].present && pg.band[c][k][b].difference != (interlaced && k < 2 && b == 2)) return fail_zero(ERR_BADSAMPLE);
	// (as decode_on_handle refuses them for intra samples: YU64 and v210 of an interlaced group at full resolution, RG24 at either, and the 16-bit-row outputs RG48 / b64a /
	// BGRA / BGRa at full resolution below 128 pixels -- BADFORMAT, zeroed picture, nothing queued; the P-frame sample behind it has no picture either)
	const bool rows16_out = d->out_kind == PIX_BGRA || d->out_kind == PIX_BGRa || d->out_kind == PIX_RG48 || d->out_kind == PIX_B64A;
	if (interlaced && ((!d->half && (d->out_kind == PIX_YU64 || d->out_kind == PIX_V210 || (rows16_out && pg.width < 128))) || d->out_kind == PIX_RG24)) {
		d->gop_second = false;
		return fail_zero(ERR_BADFORMAT);
	}
	if (d->gop_ready && d->gplan.interlaced != interlaced) d->gop_ready = false;
	d->gplan.interlaced = interlaced;
	if (!d->gop_ready) {
		device_select(d->device);
		const int prc = d->gop_batch.prepare(gp, true, d->out_kind, d->half);
		device_select(-1);
		if (prc) return ERR_INTERNAL;
		d->gop_ready = true;
	}
	// for outputs that convert YUV to RGB: 601 or 709 by the group's colour space tag, the computer-systems range (plan_from_sample)
	d->gop_batch.set_color_matrix((pg.color_space & 3) == 1 ? 2 : 0);
	const uint32_t dither_seed = 0x2545F491u * ++d->frames_decoded;
	// GPU entropy stage (the default): the sample goes to HBM, every coded band to one workgroup; a sample the device stage does not serve (launch < 0: geometry
	// the kernels do not take, a raw band with a divisor) is decoded below by the host coder instead
	if (gpu_entropy_enabled() && d->gop_batch.launch_entropy_decode(s, size, pg, (size_t)gp.width * gp.display_height * 8 + 131072) == 0) {
		if (d->gop_batch.launch_inverse(dither_seed, true)) return ERR_INTERNAL;
		if (d->gop_batch.download_frame(0, nullptr, 0) || d->gop_batch.download_frame(1, nullptr, 0) || d->gop_batch.wait()) return ERR_INTERNAL;
		if (d->gop_batch.entropy_decode_errors()) return fail_zero(ERR_BADSAMPLE);
		d->gop_batch.finish_frame(0, out, pitch);
		d->gop_second = true;
		return ERR_OKAY;
	}
	if (gpu_entropy_strict()) return fail_zero(ERR_INTERNAL);
	int16_t *coeffs = d->gop_batch.host_coeffs_rw();
	memset(coeffs, 0, gp.coeff_elems * 2);
	for (int c = 0; c < 3; c++) {
		const GopChannel &ch = gp.ch[c];
		const ParsedBand &lp = pg.lowpass[c];
		const GopWavelet &top = ch.w[5];
		if (!lp.present || lp.width != top.width || lp.height != top.height) return fail_zero(ERR_BADSAMPLE);
		// the bias the reference adds to the lowpass band while unpacking it: the group's of the requested output (group_lowpass_bias; decoder.c:12265 `num_frames == 2 ? 48 : 24`)
		const int bias = group_lowpass_bias(top.width, d->out_kind, c);
		for (int r = 0; r < top.height; r++) {
			const uint8_t *p = s + lp.offset + (size_t)r * top.width * 2;
			int16_t *dst = coeffs + top.offset[0] + (size_t)r * top.pitch;
			// (a band of odd width is read 16 unsigned bits at a time, one of even width as pairs of signed words: decoder.c:12240-12290, as k_dec_lowpass does)
			for (int x = 0; x < top.width; x++) { int v = (int16_t)((p[2 * x] << 8) | p[2 * x + 1]); if (top.width & 1) v = (int)(uint16_t)v; v += bias; dst[x] = (int16_t)(v > 0x7fff ? 0x7fff : v); }
		}
		static const int coded[5] = { 5, 4, 3, 1, 0 };
		for (int k : coded) {
			const GopWavelet &wv = ch.w[k];
			for (int b = (k == 3 ? 0 : 1); b < 4; b++) {
				const ParsedBand &pb = pg.band[c][k][b];
				if (!pb.present || pb.width != wv.width || pb.height != wv.height) return fail_zero(ERR_BADSAMPLE);
				int16_t *dst = coeffs + wv.offset[b];
				if (pb.codebook == -2) {                                     // the same band divided and coded in two passes (groups from 8-bit RGB sources: cfhd_gop.h)
					if (k != 3 || b != 0 || vlc_decode_band_two_pass(s + pb.offset, pb.bytes, wv.width, wv.height, wv.pitch, pb.quant, dst)) return fail_zero(ERR_BADSAMPLE);
				} else if (pb.codebook < 0) {                                // raw 16-bit words (the lowpass band of the temporal highpass wavelet)
					if ((size_t)pb.bytes < (size_t)wv.width * wv.height * 2) return fail_zero(ERR_BADSAMPLE);
					for (int r = 0; r < wv.height; r++) {
						const uint8_t *p = s + pb.offset + (size_t)r * wv.width * 2;
						for (int x = 0; x < wv.width; x++) dst[(size_t)r * wv.pitch + x] = (int16_t)(((p[2 * x] << 8) | p[2 * x + 1]) * pb.quant);
					}
				} else if (vlc_decode_band(s + pb.offset, pb.bytes, wv.width, wv.height, wv.pitch, pb.quant, pb.codebook, dst)) return fail_zero(ERR_BADSAMPLE);
				// interlaced groups: peak values, then every row becomes its running sum (decoder.c:19809, :20822)
				if (pb.difference) finish_difference_band(dst, wv.width, wv.height, wv.pitch, pb.peak_level ? s + pb.peak_offset : nullptr, pb.peak_level ? size - pb.peak_offset : 0, pb.peak_level);
			}
		}
	}
	if (d->gop_batch.launch_inverse(dither_seed)) return ERR_INTERNAL;
	if (d->gop_batch.download_frame(0, nullptr, 0) || d->gop_batch.download_frame(1, nullptr, 0) || d->gop_batch.wait()) return ERR_INTERNAL;
	d->gop_batch.finish_frame(0, out, pitch);
	d->gop_second = true;
	return ERR_OKAY;
}

CFHD_Error CFHD_DecodeSample(CFHD_DecoderRef ref, void *sample, size_t size, void *out, int32_t pitch)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref || !sample || !out) return ERR_INVALID_ARGUMENT;
	Decoder *d = (Decoder *)ref;
	DecodeInFlight decode_in_flight(d->device);      // (encoder pools on the same GPU gather their frames while decoders are at work there: encode_one_gathered)
	if (!d->prepared) return ERR_UNEXPECTED;
	const uint8_t *s = (const uint8_t *)sample;
	if (d->gop) return decode_group_sample(d, s, size, out, pitch);
	ParsedSample ps;
	auto fail_zero = [&](int err) {                                               // decode failure zero-fills the output (decoder.c:11850-11859)
		const int quad = d->plan.encoded_format == ENC_BAYER ? 2 : 1;      // (the plan of a Bayer sample counts photosite quads)
		const int rowbytes = packed_frame_pitch(d->out_kind, d->half ? d->plan.width / 2 : quad * d->plan.width), rows = d->half ? d->plan.display_height / 2 : quad * d->plan.display_height;
		for (int r = 0; r < rows; r++) memset((uint8_t *)out + (ptrdiff_t)r * pitch, 0, (size_t)rowbytes);
		return err;
	};
	const int parsed = parse_sample(s, size, &ps);
	if (ps.uncompressed) { device_set_last_error(kUncompressedRefusal); return fail_zero(ERR_BADFORMAT); }
	if (parsed != 0) return fail_zero(ERR_BADSAMPLE);
	if (ps.width != d->header.width || ps.display_height != d->header.display_height || ps.encoded_format != d->header.encoded_format ||
	    ps.num_channels != d->plan.num_channels) return fail_zero(ERR_BADSAMPLE);
	// interlaced samples (known only now: the SAMPLE_FLAGS tag lies behind the 512 bytes CFHD_PrepareToDecode sees): 4:2:2, full resolution through the
	// inverse frame transform, half resolution from the level-1 lowpass planes like any other sample (the reference's output is the same model)
	const bool interlaced = !ps.progressive;
	// (RG48 / b64a / BGRA / BGRa of an interlaced sample at full resolution: the reference's 16-bit rows of the inverse frame transform, decoder.c:26488 -> :22027
	// TransformInverseFrameToRow16u, then its RGB conversion of those rows, bayer.c:13186 -- k_inv_frame_yuv422_rows16 + k_yu64_to_rgb16 -- at the widths of the
	// progressive RG48-of-4:2:2 route; at half resolution the level-1 lowpass planes, as for progressive samples)
	// (YU64 / v210 output of interlaced samples: at half resolution only -- the level-1 lowpass planes, as for progressive samples; RG24 takes another route there: not built)
	// (likewise the 10-bit RGB words of an interlaced sample: half resolution only; refusing here keeps the contract of every other unsupported combination:
	// BADFORMAT, zeroed picture, nothing queued)
	const bool rows16_out = d->out_kind == PIX_BGRA || d->out_kind == PIX_BGRa || d->out_kind == PIX_RG48 || d->out_kind == PIX_B64A;
	const bool planes_out = d->out_kind == PIX_YU64 || d->out_kind == PIX_V210 || (d->out_kind >= PIX_R210 && d->out_kind <= PIX_AR10);
	if (interlaced && (ps.encoded_format != ENC_YUV422 || (planes_out && !d->half) || d->out_kind == PIX_RG24)) return fail_zero(ERR_BADFORMAT);
	if (interlaced && rows16_out && !d->half && ps.width < 128) return fail_zero(ERR_BADFORMAT);
	if (interlaced && !d->half && ps.width > 8192) return fail_zero(ERR_BADFORMAT);        // k_dec_undiff serves rows of up to 4096 coefficients (cfhd_dec_kernels.h DXU_MAX): an unsupported size, not a bad sample
	// another call of this geometry in flight right now: decode together with it (see DecodeService)
	if (decode_gather_slots() > 1 && gpu_entropy_enabled() && size <= (size_t)d->plan.width * d->plan.height * pixel_bytes_of(d->out_kind) + 65536) {
		if (!d->service || d->service_interlaced != interlaced) {
			DecodeServiceKey key; memset(&key, 0, sizeof(key));
			key.width = d->plan.width; key.height = d->plan.height; key.display_height = d->plan.display_height; key.encoded_format = d->plan.encoded_format;
			key.precision = d->plan.precision; for (int k = 0; k < 3; k++) key.prescale[k] = d->plan.prescale[k];
			key.out_kind = d->out_kind; key.half = d->half; key.interlaced = interlaced; key.device = d->device;
			d->service = decode_services().find(key); d->service_interlaced = interlaced;
		}
		DecodeService *svc = d->service;
		if (!svc) return decode_on_handle(d, ps, s, size, out, pitch, interlaced);
		struct InFlight { std::atomic<int> &n; int before; InFlight(std::atomic<int> &c) : n(c), before(c.fetch_add(1)) {} ~InFlight() { n.fetch_sub(1); } } mark(svc->inflight);
		if (mark.before > 0) {
			bool usable;
			{
				std::lock_guard<std::mutex> lk(svc->m);
				if (!svc->ok && !svc->dead) { if (!svc->start(d->plan, d->out_kind, d->half, interlaced, decode_gather_slots())) svc->dead = true; }   // (could not be set up: never tried again)
				usable = svc->ok;
			}
			if (usable && svc->decode(s, size, out, pitch) == 0) return ERR_OKAY;
			// not decoded there (damaged sample in the pass, device trouble): this handle's own path gives this sample its own verdict
		}
		return decode_on_handle(d, ps, s, size, out, pitch, interlaced);
	}
	return decode_on_handle(d, ps, s, size, out, pitch, interlaced);
}

// One sample on the handle's own batch of one frame (the only path of a caller that decodes alone).
static CFHD_Error decode_on_handle(Decoder *d, const ParsedSample &ps, const uint8_t *s, size_t size, void *out, int32_t pitch, bool interlaced)
{
	auto fail_zero = [&](int err) {                                               // decode failure zero-fills the output (decoder.c:11850-11859)
		const int quad = d->plan.encoded_format == ENC_BAYER ? 2 : 1;      // (the plan of a Bayer sample counts photosite quads)
		const int rowbytes = packed_frame_pitch(d->out_kind, d->half ? d->plan.width / 2 : quad * d->plan.width), rows = d->half ? d->plan.display_height / 2 : quad * d->plan.display_height;
		for (int r = 0; r < rows; r++) memset((uint8_t *)out + (ptrdiff_t)r * pitch, 0, (size_t)rowbytes);
		return err;
	};
	if (d->batch_ready && d->batch.interlaced() != interlaced) d->batch_ready = false;
	if (!d->batch_ready) {
		d->batch.set_interlaced(interlaced);
		device_select(d->device);                      // the handle's GPU (the batch remembers it: later calls may come from any thread)
		d->batch.set_stage_pieces(sync_stage_pieces());
		int prc = d->batch.prepare(d->plan, 1, d->out_kind, d->half);
		if (!prc && gpu_entropy_enabled()) prc = d->batch.prepare_entropy((size_t)d->plan.width * d->plan.height * pixel_bytes_of(d->out_kind) + 65536);
		device_select(-1);
		if (prc) return ERR_INTERNAL;
		d->batch_ready = true;
	}
	if (d->batch.has_entropy() && size <= (size_t)d->plan.width * d->plan.height * pixel_bytes_of(d->out_kind) + 65536) {
		// GPU entropy decoder: ship the sample bytes, the pyramid is rebuilt in HBM
		d->prof.start();
		if (d->batch.entropy().set_sample_host(0, s, size)) return fail_zero(ERR_BADSAMPLE);
		d->prof.mark(0);
		if (d->batch.launch_entropy()) return ERR_INTERNAL;
		if (d->batch.launch_inverse(0x2545F491u * ++d->frames_decoded)) return ERR_INTERNAL;
		if (d->batch.download_frame(0, out, pitch)) return ERR_INTERNAL;
		d->prof.mark(1);
		// the picture is copied out piece by piece behind the DMA of each piece (finish_frame waits on their events); whether the sample decoded cleanly is known
		// behind it -- a damaged one has its output zeroed as before
		if (d->batch.staged_in_pieces()) {
			if (d->batch.finish_frame(0, out, pitch)) return ERR_INTERNAL;
			d->prof.mark(2);
			if (d->batch.wait()) return ERR_INTERNAL;
			if (d->batch.entropy().check()) return fail_zero(ERR_BADSAMPLE);
		} else {
			if (d->batch.wait()) return ERR_INTERNAL;
			d->prof.mark(2);
			if (d->batch.entropy().check()) return fail_zero(ERR_BADSAMPLE);
			d->batch.finish_frame(0, out, pitch);
		}
		d->prof.mark(3); d->prof.calls++;
		return ERR_OKAY;
	}
	// Entropy decode on the host into the pinned coefficient staging (dequantized values, as the reference's FSM delivers them).
	d->batch.clear_host_coeffs(0);
	int16_t *coeffs = d->batch.host_coeffs(0);
	const FramePlan &plan = d->plan;
	// The reference biases the lowpass band while unpacking it (Codec/decoder.c:12240-12290 "channeloffset"):
	// see lowpass_bias().
	for (int c = 0; c < plan.num_channels; c++) {
		const ParsedBand &lp = ps.lowpass[c];
		const BandDesc &ll = plan.ch[c].band[2][0];
		if (!lp.present || lp.width != ll.width || lp.height != ll.height) return fail_zero(ERR_BADSAMPLE);
		const int lowpass_offset = lowpass_bias(plan.precision, ll.width, d->out_kind, c);
		for (int r = 0; r < ll.height; r++) {
			const uint8_t *p = s + lp.offset + (size_t)r * ll.width * 2;
			int16_t *dst = coeffs + ll.offset + (size_t)r * ll.pitch;
			for (int x = 0; x < ll.width; x++) {
				int v = (int16_t)((p[2 * x] << 8) | p[2 * x + 1]);
				if (ll.width & 1) v = (int)(uint16_t)v;           // (odd width: 16 unsigned bits at a time, decoder.c:12240-12290; the same rule as k_dec_lowpass)
				v += lowpass_offset;
				dst[x] = (int16_t)(v > 0x7fff ? 0x7fff : v);
			}
		}
		for (int lv = 0; lv < kNumLevels; lv++)
			for (int b = 1; b < 4; b++) {
				const ParsedBand &pb = ps.high[c][lv][b];
				const BandDesc &bd = plan.ch[c].band[lv][b];
				if (!pb.present || pb.width != bd.width || pb.height != bd.height) return fail_zero(ERR_BADSAMPLE);
				if (vlc_decode_band(s + pb.offset, pb.bytes, bd.width, bd.height, bd.pitch, pb.quant, pb.codebook, coeffs + bd.offset)) return fail_zero(ERR_BADSAMPLE);
				if (pb.difference) {
					if (pb.peak_level && (size_t)pb.peak_offset + 2 > size) return fail_zero(ERR_BADSAMPLE);
					finish_difference_band(coeffs + bd.offset, bd.width, bd.height, bd.pitch, pb.peak_level ? s + pb.peak_offset : nullptr, pb.peak_level ? size - pb.peak_offset : 0, pb.peak_level);
				}
			}
	}
	if (d->batch.upload_coeffs()) return ERR_INTERNAL;
	if (d->batch.launch_inverse(0x2545F491u * ++d->frames_decoded)) return ERR_INTERNAL;
	if (d->batch.download_frame(0, out, pitch)) return ERR_INTERNAL;
	if (d->batch.wait()) return ERR_INTERNAL;
	d->batch.finish_frame(0, out, pitch);
	return ERR_OKAY;
}

CFHD_Error CFHD_SetLicense(CFHD_DecoderRef ref, const unsigned char *) { return ref ? ERR_OKAY : ERR_INVALID_ARGUMENT; }
CFHD_Error CFHD_SetActiveMetadata(CFHD_DecoderRef ref, CFHD_MetadataRef, unsigned int, CFHD_MetadataType, void *, unsigned int)
{
	// Active-metadata image development (colour, 3D, burn-ins) is outside the hot path; the tags are accepted and ignored.
	return ref ? ERR_OKAY : ERR_INVALID_ARGUMENT;
}
CFHD_Error CFHD_ClearActiveMetadata(CFHD_DecoderRef ref, CFHD_MetadataRef) { return ref ? ERR_OKAY : ERR_INVALID_ARGUMENT; }
// 1/8 x 1/8 thumbnail straight from the raw lowpass bands of the sample, no decode and no GPU involved (host code as in the reference:
// Codec/thumbnail.c:65 GenerateThumbnail).  Output: 10-bit RGB, one big-endian dword per pixel, r << 22 | g << 12 | b << 2 ("DPX0").
//   4:2:2: per pixel pair, y = (lowpass >> 4 & 0x3ff) - 64, Cr / Cb = (lowpass >> 4 & 0x3ff) - 512 from channels 1 / 2, then the fixed-point
//          709 matrix of thumbnail.c:205-222;  4:4:4(:4): the G, R, B lowpass values >> 4.  Bayer samples are not built.
static int thumbnail_from_sample(const void *sample, size_t size, void *out, size_t out_size, size_t *rw, size_t *rh, size_t *rsize)
{
	if (!sample) return ERR_INVALID_ARGUMENT;
	ParsedSample ps;
	if (parse_sample((const uint8_t *)sample, size, &ps) != 0) return ERR_BADSAMPLE;
	const int enc = ps.encoded_format;
	if (enc != ENC_YUV422 && enc != ENC_RGB444 && enc != ENC_RGBA4444) return ERR_BADFORMAT;
	const int w = (ps.width + 7) / 8, h = (ps.height + 7) / 8;
	for (int c = 0; c < 3; c++) {
		const ParsedBand &lp = ps.lowpass[c];
		const int cw = (enc == ENC_YUV422 && c) ? w / 2 : w;
		if (!lp.present || lp.width != cw || lp.height != h || (size_t)lp.offset + (size_t)cw * h * 2 > size) return ERR_BADSAMPLE;
	}
	if (!out) {                                          // size query (thumbnail.c:30 GetThumbnailInfo)
		if (rw) *rw = (size_t)w;
		if (rh) *rh = (size_t)h;
		if (rsize) *rsize = (size_t)w * h * 4;
		return ERR_OKAY;
	}
	if ((w & 1) || out_size < (size_t)w * h * 4) return ERR_INVALID_ARGUMENT;
	const uint8_t *s = (const uint8_t *)sample;
	auto be16 = [&](const ParsedBand &b, size_t i) { const uint8_t *p = s + b.offset + 2 * i; return (int)((p[0] << 8) | p[1]); };
	auto clamp10 = [](int v) { return v < 0 ? 0 : (v > 0x3ff ? 0x3ff : v); };
	auto put = [&](size_t i, int r, int g, int b) {
		const uint32_t rgb = ((uint32_t)r << 22) | ((uint32_t)g << 12) | ((uint32_t)b << 2);
		uint8_t *o = (uint8_t *)out + 4 * i;
		o[0] = (uint8_t)(rgb >> 24); o[1] = (uint8_t)(rgb >> 16); o[2] = (uint8_t)(rgb >> 8); o[3] = (uint8_t)rgb;
	};
	const size_t n = (size_t)w * h;
	if (enc == ENC_YUV422) {
		for (size_t i = 0; i < n; i += 2) {
			const int cr = ((be16(ps.lowpass[1], i / 2) >> 4) & 0x3ff) - 0x200, cb = ((be16(ps.lowpass[2], i / 2) >> 4) & 0x3ff) - 0x200;
			for (int k = 0; k < 2; k++) {
				const int y = ((be16(ps.lowpass[0], i + k) >> 4) & 0x3ff) - 64;
				put(i + k, clamp10((1192 * y + 1836 * cr) >> 10), clamp10((1192 * y - 547 * cr - 218 * cb) >> 10), clamp10((1192 * y + 2166 * cb) >> 10));
			}
		}
	} else {
		for (size_t i = 0; i < n; i++)
			put(i, (be16(ps.lowpass[1], i) >> 4) & 0x3ff, (be16(ps.lowpass[0], i) >> 4) & 0x3ff, (be16(ps.lowpass[2], i) >> 4) & 0x3ff);
	}
	if (rw) *rw = (size_t)w;
	if (rh) *rh = (size_t)h;
	if (rsize) *rsize = n * 4;
	return ERR_OKAY;
}

CFHD_Error CFHD_GetThumbnail(CFHD_DecoderRef ref, void *sample, size_t size, void *out, size_t out_size, uint32_t, size_t *rw, size_t *rh, size_t *rsize)
{
	if (!ref || !sample || !out) return ERR_INVALID_ARGUMENT;
	return thumbnail_from_sample(sample, size, out, out_size, rw, rh, rsize);
}

// EncoderSDK/CFHDEncoder.cpp:593: the same thumbnail, asked of an encoder for a sample it produced.
CFHD_Error CFHD_GetEncodeThumbnail(CFHD_EncoderRef ref, void *sample, size_t size, void *out, size_t out_size, uint32_t, size_t *rw, size_t *rh, size_t *rsize)
{
	if (!ref || !sample || !out) return ERR_INVALID_ARGUMENT;
	return thumbnail_from_sample(sample, size, out, out_size, rw, rh, rsize);
}

// EncoderSDK/CFHDEncoderPool.cpp:620: thumbnail of a sample buffer of the encoder pool; without an output buffer only the dimensions.
CFHD_Error CFHD_GetSampleThumbnail(CFHD_SampleBufferRef ref, void *out, size_t out_size, uint32_t, uint_least16_t *rw, uint_least16_t *rh,
                                   CFHD_PixelFormat *fmt, size_t *rsize)
{
	if (!ref) return ERR_INVALID_ARGUMENT;
	SampleBuffer *sb = (SampleBuffer *)ref;
	size_t w = 0, h = 0, n = 0;
	const int rc = thumbnail_from_sample(sb->data.data(), sb->size, out_size ? out : nullptr, out_size, &w, &h, &n);
	if (rc != ERR_OKAY) return ERR_CODEC_ERROR;
	if (rw) *rw = (uint_least16_t)w;
	if (rh) *rh = (uint_least16_t)h;
	if (fmt) *fmt = FOURCC_BE('D', 'P', 'X', '0');
	if (rsize) *rsize = n;
	return ERR_OKAY;
}

// DecoderSDK/CFHDDecoder.cpp:443 (obsoleted there by CFHD_GetSampleInfo): encoded format, field type and frame size of a sample.  The
// reference's CFHD_SampleHeader is a class of exactly these four ints (Common/CFHDSampleHeader.h:32).
CFHD_Error CFHD_ParseSampleHeader(void *sample, size_t size, CFHD_SampleHeader *hdr)
{
	if (!sample || !hdr) return ERR_INVALID_ARGUMENT;
	ParsedSample ps;
	if (parse_sample((const uint8_t *)sample, size, &ps) < 0) return ERR_BADSAMPLE;
	hdr->encoded_format = ps.encoded_format == ENC_RGB444 ? 1 : (ps.encoded_format == ENC_RGBA4444 ? 2 : (ps.encoded_format == ENC_BAYER ? 3 : 0));
	// CSampleDecoder::FieldType (SampleDecoder.cpp:1886): 1 progressive; interlaced: 2 upper field first unless the optional interlaced
	// flags say interlaced (bit 0) without field-1-first (bit 1), then 3 lower field first
	if (ps.progressive || ps.encoded_format == ENC_BAYER) hdr->field_type = 1;
	else hdr->field_type = ((ps.interlaced_flags & 1) && !(ps.interlaced_flags & 2)) ? 3 : 2;
	hdr->width = ps.width; hdr->height = ps.display_height;
	return ERR_OKAY;
}

CFHD_Error CFHD_CloseDecoder(CFHD_DecoderRef ref)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref) return ERR_INVALID_ARGUMENT;
	static const char *const names[] = { "parse+stage", "submit", "gpu+copies", "copy out" };
	((Decoder *)ref)->prof.report("CFHD_DecodeSample", names, 4);
	delete (Decoder *)ref;
	return ERR_OKAY;
}
