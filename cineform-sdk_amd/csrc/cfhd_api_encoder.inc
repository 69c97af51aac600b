// cfhd_api_encoder.inc -- part of cfhd_api.cpp (one translation unit: the parts are #included there in this order, they share the handle types of an unnamed namespace).
// CFHD_OpenEncoder ... CFHD_CloseEncoder (Common/CFHDEncoder.h:254-310; EncoderSDK/CFHDEncoder.cpp, SampleEncoder.cpp).

// =============================================================================================
// Synchronous encoder
// =============================================================================================
CFHD_Error CFHD_OpenEncoder(CFHD_EncoderRef *out, CFHD_ALLOCATOR *)
{
	if (!out) return ERR_INVALID_ARGUMENT;
	Encoder *e = new (std::nothrow) Encoder;
	if (!e) return ERR_OUTOFMEMORY;
	*out = e;
	return ERR_OKAY;
}

CFHD_Error CFHD_GetInputFormats(CFHD_EncoderRef ref, CFHD_PixelFormat *arr, int len, int *count)
{
	if (!ref || !arr) return ERR_INVALID_ARGUMENT;
	const uint32_t fmts[] = { FMT_YUY2, FMT_2VUY, FMT_RG48, FMT_B64A, FMT_BYR4, FMT_YU64, FMT_V210, FMT_RG24, FMT_BGRA, FMT_BGRa, FMT_R210, FMT_DPX0, FMT_AB10, FMT_AR10, FMT_RG30, FMT_BYR5, FMT_RG64 };
	int n = 0;
	for (; n < (int)(sizeof(fmts) / sizeof(fmts[0])) && n < len; n++) arr[n] = fmts[n];
	if (count) *count = n;
	return ERR_OKAY;
}

CFHD_Error CFHD_PrepareToEncode(CFHD_EncoderRef ref, int w, int h, CFHD_PixelFormat fmt, CFHD_EncodedFormat encoded,
                                CFHD_EncodingFlags flags, CFHD_EncodingQuality quality)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref) return ERR_INVALID_ARGUMENT;
	Encoder *e = (Encoder *)ref;
	const int want_encoded = e->params.encoded_format == ENC_RGB444 ? 1 : (e->params.encoded_format == ENC_RGBA4444 ? 2 : (e->params.encoded_format == ENC_BAYER ? 3 : 0));
	if (e->params.valid && e->params.width == w && e->params.height == h && e->params.pixel_format == fmt && e->params.flags == (uint32_t)flags &&
	    want_encoded == (int)encoded) {
		// "just changing quality" (SampleEncoder.cpp:322-327); a different encoded format or other flags take the full path below
		if (quality_word_refused(e->params.pixel_kind, (int)quality)) return ERR_BADFORMAT;      // (as make_params refuses it; the handle keeps what it was prepared with)
		e->params.quality = (int)((0xffff0000u & (uint32_t)e->params.quality) | (0xffffu & (uint32_t)quality));
		derive_quantization(&e->params.plan, e->params.quality, e->params.progressive, 0.0f, &e->params.qstate);
		e->batch_ready = false;
		// (a group encoder deals its tables on the call that opens the next group, from e->params.quality: nothing to do here)
		return ERR_OKAY;
	}
	int rc = make_params(e->params, w, h, fmt, encoded, flags, quality);
	if (rc) return rc;
	e->batch_ready = false;
	e->frame_number = 0;
	e->sample.assign(sample_capacity(e->params), 0);
	e->sample_size = 0;
	e->gop_calls = 0; e->gop_ready = false;
	return ERR_OKAY;
}

// The group encoder's device side, on the first call that needs it: the group batch, a sample buffer for two frames, the GPU entropy stage.
static int prepare_group_encoder(Encoder *e)
{
	if (e->gop_ready) return 0;
	if (e->gop_batch.prepare(e->params.gplan, false, e->params.pixel_kind)) return -1;
	e->gop_ready = true;
	e->sample.assign(2 * sample_capacity(e->params), 0);
	// (a group whose w[3] lowpass band is divided and coded in two passes -- the 8-bit RGB inputs, cfhd_gop.h gop_temporal_lowpass_is_coded -- takes the device stage
	// too: k_ent_split_two_pass in front of the count stage)
	if (gpu_entropy_enabled() && e->gop_batch.prepare_entropy(e->sample.size())) return -1;
	return 0;
}

CFHD_Error CFHD_SetEncodeLicense(CFHD_EncoderRef ref, unsigned char *) { return ref ? ERR_OKAY : ERR_INVALID_ARGUMENT; }
CFHD_Error CFHD_SetEncodeLicense2(CFHD_EncoderRef ref, unsigned char *, uint32_t *level) { if (level) *level = 31; return ref ? ERR_OKAY : ERR_INVALID_ARGUMENT; }

CFHD_Error CFHD_EncodeSample(CFHD_EncoderRef ref, void *frame, int pitch)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref || !frame) return ERR_INVALID_ARGUMENT;
	Encoder *e = (Encoder *)ref;
	if (!e->params.valid) return ERR_CODEC_ERROR;
	e->meta.handle();
	if (e->params.gop) {
		// Two frames per sample (encoder.c:3282-3380): the first call of a sequence answers with the sequence header, the call that completes a
		// pair with the group, the calls in between with the header of the group's second frame.  Frame numbers: group g carries 2 g + 1,
		// and so does the P-frame header behind it (pinned on the reference's samples).
		if (prepare_group_encoder(e)) return ERR_INTERNAL;
		const uint32_t n = e->gop_calls++;
		// Rate feedback: this call's step of the walk the frame queue's group streams take too (cfhd_gop.h gop_quant_call)
		bool changed = false;
		if (!gop_quant_call(&e->params.gplan, e->params.quality, &e->params.gstate, !(n & 1u), &changed)) return ERR_INTERNAL;
		if (changed) e->gop_batch.set_plan(e->params.gplan);
		if (e->gop_batch.upload_frame((int)(n & 1u), frame, pitch)) return ERR_INTERNAL;
		size_t bytes;
		if (!(n & 1u)) {
			if (e->gop_batch.wait()) return ERR_INTERNAL;              // the caller's frame is borrowed for the call only: it is in pinned memory now
			bytes = n == 0 ? write_sequence_header(e->params.gplan, gop_sequence_input_format(e->params.pixel_kind, color_format_of(e->params.pixel_kind)), e->sample.data(), e->sample.size())
			               : write_pframe_sample(e->params.gplan, n - 1, e->sample.data(), e->sample.size());
		} else {
			MetaBlock global = e->meta.global, local = e->meta.local;
			meta_remove_hidden(global); meta_remove_hidden(local);
			SampleHeaderInfo hdr = { n, color_format_of(e->params.pixel_kind), e->params.color_space, header_quality(e->params.quality), !e->params.gplan.interlaced, global.data(), global.size(), local.data(), local.size() };
			if (e->gop_batch.launch_forward()) return ERR_INTERNAL;
			bytes = 0;
			// GPU entropy stage: the finished group sample comes back, not the pyramid.  The host writer takes over (from the same GPU coefficients) when the header
			// does not fit the device template block, and for a sample so large that the reference would have zeroed bands of the frame wavelets (encoder.c:8332:
			// that depends on the bytes written so far, which the device stage only knows when it is done)
			if (e->gop_batch.has_entropy() && e->gop_batch.entropy().set_frame_header(0, hdr) == 0) {
				if (e->gop_batch.entropy().launch() || e->gop_batch.entropy().download() || e->gop_batch.wait()) return ERR_INTERNAL;
				const size_t nb = e->gop_batch.entropy().sample_bytes(0);
				// (an interlaced group with more peak values in a difference-coded band than the entropy stage's positions hold: the host writer's, as for interlaced intra frames)
				if (nb && nb <= e->sample.size() && !gop_sample_may_zero_bands(e->params.gplan, nb) && !e->gop_batch.entropy().needs_peak_table(0)) { memcpy(e->sample.data(), e->gop_batch.entropy().host_sample(0), nb); bytes = nb; }
			}
			if (!bytes) {
				if (gpu_entropy_strict()) return ERR_INTERNAL;
				if (e->gop_batch.download_coeffs() || e->gop_batch.wait()) return ERR_INTERNAL;
				bytes = write_group_sample(e->params.gplan, hdr, e->gop_batch.host_coeffs(), e->sample.data(), e->sample.size());
			}
		}
		e->meta.local.clear();
		if (!bytes) return ERR_CODEC_ERROR;
		e->sample_size = bytes;
		if (n == 0 || (n & 1u)) gop_quant_key_sample(&e->params.gstate, bytes);      // key samples: the sequence header and the groups (encoder.c:3414)
		return ERR_OKAY;
	}
	if (!e->batch_ready) {
		e->batch.set_stage_pieces(sync_stage_pieces());
		if (prepare_batch(e->batch, e->params)) return ERR_INTERNAL;
		e->batch_ready = true;
	}
	e->prof.start();
	int rc = encode_one(e->batch, e->params, frame, pitch, ++e->frame_number, e->meta.global, e->meta.local,
	                    e->sample.data(), e->sample.size(), &e->sample_size);
	e->prof.mark(0); e->prof.calls++;
	e->meta.local.clear();                                                // FreeLocalMetadata (CFHDEncoder.cpp:351)
	return rc;
}

// Extension: the level-1 transform kernel behind the handle's next CFHD_EncodeSample (as a profiler shows it), "" before CFHD_PrepareToEncode.  A group encoder answers
// from GopBatch::forward_route(), an intra encoder from EncodeBatch::forward_route(): the routes the launches themselves read.
const char *cfhd_amd_encoder_kernel_name(CFHD_EncoderRef ref)
{
	CallerDevice caller_device;
	if (!ref || *(const uint32_t *)ref != kEncoderMagic) return "";
	Encoder *e = (Encoder *)ref;
	if (!e->params.valid) return "";
	if (e->params.gop) {
		if (prepare_group_encoder(e)) return "";
		return e->gop_batch.level1_kernel();
	}
	if (!e->batch_ready) {
		e->batch.set_stage_pieces(sync_stage_pieces());
		if (prepare_batch(e->batch, e->params)) return "";
		e->batch_ready = true;
	}
	return e->batch.level_kernel(0, true);      // (encode_one launches with the coefficients kept)
}

CFHD_Error CFHD_GetSampleData(CFHD_EncoderRef ref, void **data, size_t *size)
{
	if (!ref || !data || !size) return ERR_INVALID_ARGUMENT;
	Encoder *e = (Encoder *)ref;
	*data = e->sample.data(); *size = e->sample_size;
	return ERR_OKAY;
}

CFHD_Error CFHD_ReleaseEncoderPool(CFHD_EncoderPoolRef ref);
CFHD_Error CFHD_CloseEncoder(CFHD_EncoderRef ref)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref) return ERR_INVALID_ARGUMENT;
	if (*(const uint32_t *)ref == kPoolMagic) return CFHD_ReleaseEncoderPool((CFHD_EncoderPoolRef)ref);      // (what the reference's harness does on its error path)
	if (*(const uint32_t *)ref != kEncoderMagic) return ERR_INVALID_ARGUMENT;
	static const char *const names[] = { "encode_one" };
	((Encoder *)ref)->prof.report("CFHD_EncodeSample", names, 1);
	delete (Encoder *)ref;
	return ERR_OKAY;
}
