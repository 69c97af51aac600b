// cfhd_api_pool.inc -- part of cfhd_api.cpp (one translation unit: the parts are #included there in this order, they share the handle types of an unnamed namespace).
// CFHD_CreateEncoderPool ... CFHD_ReleaseEncoderPool (Common/CFHDEncoder.h:338-427; EncoderSDK/CFHDEncoderPool.cpp, EncoderPool.cpp:239-380, AsyncEncoder.cpp).

// =============================================================================================
// Asynchronous encoder pool
// =============================================================================================
CFHD_Error CFHD_CreateEncoderPool(CFHD_EncoderPoolRef *out, int threads, int queue_len, CFHD_ALLOCATOR *)
{
	if (!out) return ERR_INVALID_ARGUMENT;
	EncoderPool *p = new (std::nothrow) EncoderPool;
	if (!p) return ERR_OUTOFMEMORY;
	p->nworkers = threads > 0 ? threads : 1;
	p->queue_len = queue_len > 0 ? queue_len : p->nworkers;
	*out = p;
	return ERR_OKAY;
}

CFHD_Error CFHD_GetAsyncInputFormats(CFHD_EncoderPoolRef ref, CFHD_PixelFormat *arr, int len, int *count)
{
	if (!ref) return ERR_INVALID_ARGUMENT;
	return CFHD_GetInputFormats((CFHD_EncoderRef)ref, arr, len, count);
}

CFHD_Error CFHD_PrepareEncoderPool(CFHD_EncoderPoolRef ref, uint_least16_t w, uint_least16_t h, CFHD_PixelFormat fmt,
                                   CFHD_EncodedFormat encoded, CFHD_EncodingFlags flags, CFHD_EncodingQuality quality)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref) return ERR_INVALID_ARGUMENT;
	EncoderPool *p = (EncoderPool *)ref;
	if (p->started) {
		// A pool that is encoding takes the quality of its NEXT frames from this call and nothing else (EncoderSDK/EncoderPool.cpp:129-132 SetNextFrameQuality; the
		// reference's own harness calls this once per loop turn until its first sample comes back, Example/TestCFHD.cpp:860-897).  Frames already submitted keep the
		// tables they were submitted under: the call waits for them, then every worker takes the new tables.
		if ((int)quality == p->params.api_quality) return ERR_OKAY;
		EncodeParams np;
		const int rc = make_params(np, p->params.width, p->params.height, p->params.pixel_format, p->params.api_encoded, p->params.flags, quality);
		if (rc) return rc;
		std::unique_lock<std::mutex> lk(p->m);
		p->cv_done.wait(lk, [&] { for (auto &j : p->fifo) if (!j->finished) return false; return true; });
		p->params = np; p->service = nullptr;           // (shared passes are keyed by quality: the workers go on alone)
		// The reference hands the word to its workers as a per-frame override (EncoderSDK/AsyncEncoder.h:102, SampleEncoder.cpp:488-492): a worker's encoder is not
		// prepared again, so it keeps the limiter it was seeded with by the first prepare and the size of its last sample, and the next frame's derivation moves the
		// feedback once.  The derivation here runs on a copy of the state with no previous sample, so that it moves nothing: its tables are the ones a worker that
		// has not encoded a frame yet uses for its first; every other worker's encode_one derives them again from its own last sample before the next frame.
		// (Pinned against the reference's pool with one worker; with more, each worker carries its own state, here as there.)
		for (auto &wk : p->workers) {
			device_select(wk->device);
			EncodeParams wp = np;
			QuantState probe = wk->params.qstate; probe.lastgopbitcount = 0;
			derive_quantization(&wp.plan, wp.quality, wp.progressive, 0.0f, &probe);
			wp.qstate = wk->params.qstate;
			wk->params = wp;
			const int urc = wk->batch.update_quant(wp.plan);
			device_select(-1);
			if (urc) return ERR_INTERNAL;
		}
		return ERR_OKAY;
	}
	if ((uint32_t)flags & 2u) return ERR_BADFORMAT;      // two-frame groups are sequential (a frame pair per sample): the synchronous encoder serves them
	return make_params(p->params, w, h, fmt, encoded, flags, quality);
}

CFHD_Error CFHD_SetEncoderPoolLicense(CFHD_EncoderPoolRef ref, unsigned char *) { return ref ? ERR_OKAY : ERR_INVALID_ARGUMENT; }
CFHD_Error CFHD_SetEncoderPoolLicense2(CFHD_EncoderPoolRef ref, unsigned char *, uint32_t *level) { if (level) *level = 31; return ref ? ERR_OKAY : ERR_INVALID_ARGUMENT; }

CFHD_Error CFHD_AttachEncoderPoolMetadata(CFHD_EncoderPoolRef ref, CFHD_MetadataRef mref)
{
	if (!ref || !mref) return ERR_INVALID_ARGUMENT;
	EncoderPool *p = (EncoderPool *)ref; EncMetadata *m = (EncMetadata *)mref;
	std::lock_guard<std::mutex> lk(m->lock);
	std::lock_guard<std::mutex> lk2(p->m);
	p->meta.global = m->global; p->meta.local = m->local;
	return ERR_OKAY;
}

CFHD_Error CFHD_StartEncoderPool(CFHD_EncoderPoolRef ref)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref) return ERR_INVALID_ARGUMENT;
	EncoderPool *p = (EncoderPool *)ref;
	if (!p->params.valid) return ERR_ENCODING_NOT_STARTED;
	if (p->started) return ERR_UNEXPECTED;               // (EncoderSDK/EncoderPool.cpp:187-189; the pool keeps running)
	p->stopping = false;
	p->workers.clear();
	for (int i = 0; i < p->nworkers; i++) {
		std::unique_ptr<PoolWorker> w(new PoolWorker);
		// the workers spread over the GPUs of the node round robin (one process per GPU -- CFHD_AMD_DEVICE / LOCAL_RANK set -- keeps them all on
		// its own); every worker owns its stream, tables and scratch on its device; delivery stays in submission order (the FIFO below)
		w->device = device_of_unit(i);
		device_select(w->device);
		const int prc = prepare_batch(w->batch, p->params);
		device_select(-1);
		if (prc) return ERR_INTERNAL;
		w->params = p->params;
		p->workers.push_back(std::move(w));
	}
	p->service = nullptr;
	bool one_device = true;
	for (auto &w : p->workers) if (w->batch.device() != p->workers[0]->batch.device()) one_device = false;
	if (one_device && encode_gather_slots() > 1 && p->nworkers > 1 && gpu_entropy_enabled() && quantizer_is_static(p->params)) {
		EncodeServiceKey key; memset(&key, 0, sizeof(key));
		key.width = p->params.width; key.height = p->params.height; key.pixel_kind = p->params.pixel_kind; key.encoded_format = p->params.encoded_format;
		key.quality = p->params.quality; key.color_space = p->params.color_space; key.flags = p->params.flags;
		key.device = p->workers[0]->batch.device();
		p->service = encode_services().find(key);
	}
	for (auto &w : p->workers) { PoolWorker *pw = w.get(); pw->thread = std::thread([p, pw] { p->worker_loop(pw); }); }
	p->started = true;
	return ERR_OKAY;
}

CFHD_Error CFHD_StopEncoderPool(CFHD_EncoderPoolRef ref)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref) return ERR_INVALID_ARGUMENT;
	((EncoderPool *)ref)->stop();
	return ERR_OKAY;
}

CFHD_Error CFHD_EncodeAsyncSample(CFHD_EncoderPoolRef ref, uint32_t frame_number, void *frame, intptr_t pitch, CFHD_MetadataRef mref)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref || !frame) return ERR_INVALID_ARGUMENT;
	EncoderPool *p = (EncoderPool *)ref;
	if (!p->started) return ERR_ENCODING_NOT_STARTED;
	std::shared_ptr<PoolJob> job(new PoolJob);
	job->frame_number = frame_number; job->frame = frame; job->pitch = pitch;    // the frame is borrowed, not copied (EncoderPool.cpp:262)
	{
		std::unique_lock<std::mutex> lk(p->m);
		// Bounded queue: block the submitter while jobQueueLength jobs are pending (MessageQueue semantics).
		p->cv_done.wait(lk, [&] { size_t pending = 0; for (auto &j : p->fifo) if (!j->finished) pending++; return pending < (size_t)p->queue_len + p->nworkers; });
		if (mref) {
			EncMetadata *m = (EncMetadata *)mref;
			std::lock_guard<std::mutex> lk2(m->lock);
			p->meta.global = m->global; p->meta.local = m->local; m->local.clear();
		}
		p->meta.handle();
		job->global = p->meta.global; job->local = p->meta.local;
		p->meta.local.clear();
		p->fifo.push_back(job);
		PoolWorker *w = p->workers[p->next_worker].get();
		p->next_worker = (p->next_worker + 1) % p->nworkers;                      // round robin on every (key) frame, EncoderPool.cpp:281-291
		w->inbox.push_back(job);
	}
	p->cv_work.notify_all();
	return ERR_OKAY;
}

static CFHD_Error pool_pop(EncoderPool *p, uint32_t *frame_number, CFHD_SampleBufferRef *out, bool wait)
{
	std::unique_lock<std::mutex> lk(p->m);
	if (p->fifo.empty()) return ERR_UNEXPECTED;
	if (!p->fifo.front()->finished) {
		if (!wait) return ERR_NOT_FINISHED;
		p->cv_done.wait(lk, [&] { return p->fifo.front()->finished; });
	}
	std::shared_ptr<PoolJob> job = p->fifo.front();
	p->fifo.pop_front();
	lk.unlock();
	p->cv_done.notify_all();
	if (frame_number) *frame_number = job->frame_number;
	if (job->error) return job->error;
	if (out) *out = job->sample.release();
	return ERR_OKAY;
}

CFHD_Error CFHD_WaitForSample(CFHD_EncoderPoolRef ref, uint32_t *frame_number, CFHD_SampleBufferRef *out)
{
	if (!ref) return ERR_INVALID_ARGUMENT;
	return pool_pop((EncoderPool *)ref, frame_number, out, true);
}

CFHD_Error CFHD_TestForSample(CFHD_EncoderPoolRef ref, uint32_t *frame_number, CFHD_SampleBufferRef *out)
{
	if (!ref) return ERR_INVALID_ARGUMENT;
	return pool_pop((EncoderPool *)ref, frame_number, out, false);
}

CFHD_Error CFHD_GetEncodedSample(CFHD_SampleBufferRef ref, void **data, size_t *size)
{
	if (!ref || !data || !size) return ERR_INVALID_ARGUMENT;
	SampleBuffer *s = (SampleBuffer *)ref;
	*data = s->data.data(); *size = s->size;
	return ERR_OKAY;
}

CFHD_Error CFHD_ReleaseSampleBuffer(CFHD_EncoderPoolRef, CFHD_SampleBufferRef ref)
{
	if (!ref) return ERR_INVALID_ARGUMENT;
	delete (SampleBuffer *)ref;
	return ERR_OKAY;
}

CFHD_Error CFHD_ReleaseEncoderPool(CFHD_EncoderPoolRef ref)
{
	CallerDevice caller_device;                      // (the caller's current HIP device is put back on the way out)
	if (!ref) return ERR_INVALID_ARGUMENT;
	EncoderPool *p = (EncoderPool *)ref;
	p->stop();
	delete p;
	return ERR_OKAY;
}
