#!/usr/bin/env python3
"""Thumbnail batches of the decode queue (cfhd_amd_decode_batch_create_thumbnails): what a pass costs and what the queue makes of it, at 1920 x 1080 YUY2, FILMSCAN1
(32 distinct frames encoded once by the product), `n` samples a pass, the samples resident in HBM unless said otherwise.  The method is the sibling tools'
(tools/rgb_as_yuv_throughput.py); the yardsticks are existing code measured in the same call:
  kernels   cfhd_amd_decode_batch_kernel_ms of ONE thumbnail batch alone -- 0 k_dec_ingest, 1 k_dec_parse, 6 k_dec_thumbnail, 9 the deliver kernel --, the variants
            alternated pass by pass, `passes` passes each: no delivery, PACKED (k_dec_deliver), RGB10_U16 / _F16 / _F32 (k_dec_deliver_rgb10); and the share of
            k_dec_ingest in the three kernels of a pass (it copies whole samples, of which a thumbnail needs the tag stream and the lowpass bands).
  queue     thumbnails per second, runs sized by TIME (`window` seconds), `repeats` runs each, run after run in turn: from HBM (submit_device) with one batch and with
            `depth` batches in flight, with RGB10_F16 delivery, and from registered host memory (submit_host, the pictures to registered host memory);
            beside them (a) the existing decode queue decoding the same samples to YUY2 from HBM, `depth` batches in flight, pictures per second, and
            (b) a loop of CFHD_GetThumbnail over the same samples on the host, one thread and 16 threads (a decoder handle each).
Medians with min .. max.  The run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end, also written to `out` when given.
`emulated` as the last argument rehearses the whole tool on the CPU (cfhd_testlib.emulated_product) at 192 x 96 with 8 samples: the numbers mean nothing there.
  python tools/thumbnail_queue_throughput.py [n=512] [depth=2] [window=2] [repeats=3] [passes=9] [limit=900] [out] [emulated]"""
import ctypes, json, os, signal, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import decode_queue as DQ
import thumbnail_queue as TQ
from planar_frames_throughput import Hbm
from yuv422_planes_throughput import stats, timed

V = ctypes.c_void_p
OFF = -1
NAMES = {OFF: "no_delivery", TQ.PACKED: "packed", TQ.RGB10_U16: "rgb10_u16", TQ.RGB10_F16: "rgb10_f16", TQ.RGB10_F32: "rgb10_f32"}


def host_loop(L, samples, nthreads, seconds):
    """Thumbnails per second of CFHD_GetThumbnail over the samples, dealt to nthreads threads (ctypes releases the interpreter lock inside the call)."""
    L.CFHD_GetThumbnail.argtypes = TQ._THUMB_ARGS
    buffers = [ctypes.create_string_buffer(s, len(s)) for s in samples]
    def work(k, counts, stop):
        dec = V(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
        out = np.zeros(1024 * 64 * 4, np.uint8); w = ctypes.c_size_t(); h = ctypes.c_size_t(); n = ctypes.c_size_t()
        done = 0
        while not stop.is_set():
            for i in range(k, len(samples), nthreads):
                assert L.CFHD_GetThumbnail(dec, buffers[i], len(samples[i]), out.ctypes.data_as(V), out.size, 0, ctypes.byref(w), ctypes.byref(h), ctypes.byref(n)) == 0
                done += 1
            counts[k] = done
        L.CFHD_CloseDecoder(dec)
    counts = [0] * nthreads; stop = threading.Event()
    threads = [threading.Thread(target=work, args=(k, counts, stop)) for k in range(nthreads)]
    t0 = time.perf_counter()
    for t in threads: t.start()
    time.sleep(max(seconds, 0.05)); stop.set()
    for t in threads: t.join()
    return sum(counts) / (time.perf_counter() - t0)


def main():
    emulated = sys.argv[-1] == "emulated"
    args = [a for a in sys.argv[1:] if a != "emulated"]
    arg = lambda k, d: int(args[k]) if len(args) > k and args[k] != "-" else d
    n, depth, window, repeats, passes, limit = arg(0, 512), arg(1, 2), arg(2, 2), arg(3, 3), arg(4, 9), arg(5, 900)
    out_path = args[6] if len(args) > 6 and args[6] != "-" else None
    signal.alarm(limit)                                   # the default action ends the process
    W, H, distinct = (1920, 1080, 32) if not emulated else (192, 96, 4)
    if emulated: n, window, passes = min(n, 8), 0, min(passes, 2)
    ctx = T.emulated_product() if emulated else None
    if ctx: ctx.__enter__()
    L = TQ.lib()
    hbm = Hbm(emulated)
    frames = [np.ascontiguousarray(T.synth_yuy2(W, H, 40 + i)[0]) for i in range(distinct)]
    unique = T.amd_encode_frames(frames, W * 2, W, H, T.PIX_YUY2, T.ENCODED_YUV422, T.QUALITY_FILMSCAN1, 0)
    del frames
    samples = [unique[i % len(unique)] for i in range(n)]
    blob, offsets, sizes = DQ.pack(samples)
    c_off, c_size = DQ._sizes(offsets), DQ._sizes(sizes)
    owner, dptr = DQ.device_copy(blob)
    if dptr is None: dptr = owner.ptr
    W8, H8 = (W + 7) // 8, (H + 7) // 8
    result = {"geometry": "%dx%d YUY2 FILMSCAN1 samples (%d distinct, %d bytes on average), thumbnails %dx%d" % (W, H, len(unique), sum(map(len, unique)) // len(unique), W8, H8),
              "samples_a_pass": n, "emulated": emulated}

    def geometry(layout):
        """(stride, pitch) of the contiguous picture of a layout."""
        if layout == TQ.PACKED: return 4 * W8 * H8, 4 * W8
        row = (W8 * TQ.ELEMENT[layout] + 15) & ~15
        return 3 * H8 * row, row

    def set_delivery(q, target, layout):
        if layout == OFF: rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0)
        else: rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, target, geometry(layout)[0], geometry(layout)[1], layout)
        assert rc == 0, T.amd_last_error()

    def submit(q): assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, c_off, c_size, n) == 0, T.amd_last_error()
    def wait(q): assert L.cfhd_amd_decode_batch_wait(q.b, None) == n, T.amd_last_error()

    queues = [TQ.ThumbQueue(unique[0], n) for _ in range(depth)]
    tensors = [hbm.alloc(n * geometry(TQ.RGB10_F32)[0]) for _ in range(depth)]

    # ---- kernels: one batch alone, the variants alternated pass by pass
    variants = [OFF, TQ.PACKED, TQ.RGB10_U16, TQ.RGB10_F16, TQ.RGB10_F32]
    ms = {NAMES[v]: {k: [] for k in (0, 1, 6, 9)} for v in variants}
    q = queues[0]
    for r in range(passes + 1):                               # (round 0: warm-up of every shape)
        for v in variants:
            set_delivery(q, tensors[0], v); submit(q); wait(q)
            if r:
                for k in (0, 1, 6, 9): ms[NAMES[v]][k].append(float(L.cfhd_amd_decode_batch_kernel_ms(q.b, k)))
    kernels = {"what": "cfhd_amd_decode_batch_kernel_ms of one thumbnail batch alone, variants alternated pass by pass, %d passes each: ms per %d thumbnails, median (min .. max)" % (passes, n)}
    for v in variants:
        row = ms[NAMES[v]]
        kernels[NAMES[v]] = {"k_dec_ingest": stats(row[0]), "k_dec_parse": stats(row[1]), "k_dec_thumbnail": stats(row[6]),
                             "deliver": dict(stats(row[9]), kernel="" if v == OFF else ("k_dec_deliver" if v == TQ.PACKED else "k_dec_deliver_rgb10"))}
    every = [ms[NAMES[v]] for v in variants]
    ingest, parse, thumb = (float(np.median(sum((row[k] for row in every), []))) for k in (0, 1, 6))
    kernels["ingest_share_of_the_three_kernels"] = round(ingest / (ingest + parse + thumb), 3) if ingest + parse + thumb > 0 else None
    kernels["sample_bytes_a_pass"] = int(sum(sizes)); kernels["lowpass_bytes_a_pass"] = n * W8 * H8 * 4      # (4:2:2: 2 bytes of luma + 2 of chroma a thumbnail pixel)
    result["kernels"] = kernels
    print("kernels", json.dumps(kernels), flush=True)

    # ---- queue: thumbnails per second beside the existing code's pictures per second
    host_pics = [np.zeros(n * 4 * W8 * H8, np.uint8) for _ in range(depth)]
    register = lambda a: L.cfhd_amd_register_host_buffer(a.ctypes.data_as(V), a.nbytes)
    assert register(blob) == 0
    for a in host_pics: assert register(a) == 0
    decoders = [DQ.Queue(unique[0], "YUY2", DQ.FULL, n) for _ in range(depth)]

    def device_round(qs):
        for k in qs: submit(k)
        for k in qs: wait(k)
        return len(qs) * n
    def host_round():
        for k, qq in enumerate(queues): assert L.cfhd_amd_decode_batch_submit_host(qq.b, blob.ctypes.data_as(V), c_off, c_size, n, host_pics[k].ctypes.data_as(V), 4 * W8 * H8, 4 * W8) == 0, T.amd_last_error()
        for qq in queues: wait(qq)
        return depth * n
    def deliver(layout):
        for k, qq in enumerate(queues): set_delivery(qq, tensors[k], layout)
    legs = [("thumbnails_from_hbm_1_batch", lambda: deliver(OFF), lambda: device_round(queues[:1])),
            ("thumbnails_from_hbm_%d_batches" % depth, lambda: deliver(OFF), lambda: device_round(queues)),
            ("thumbnails_from_hbm_%d_batches_rgb10_f16" % depth, lambda: deliver(TQ.RGB10_F16), lambda: device_round(queues)),
            ("thumbnails_from_registered_host_memory_%d_batches" % depth, lambda: deliver(OFF), host_round),
            ("a_decode_queue_yuy2_from_hbm_%d_batches" % depth, lambda: None, lambda: device_round(decoders))]
    fps = {name: [] for name, _, _ in legs}
    for r in range(repeats + 1):                              # (round 0: warm-up, not recorded)
        for name, prepare, step in legs:
            prepare()
            v = timed(step, window if r else 0)
            if r: fps[name].append(v)
        if r: print("repeat", r, {k: round(v[-1], 1) for k, v in fps.items()}, flush=True)
    for k in decoders: k.close()
    for k in queues: k.close()
    L.cfhd_amd_unregister_host_buffer(blob.ctypes.data_as(V))
    for a in host_pics: L.cfhd_amd_unregister_host_buffer(a.ctypes.data_as(V))
    hbm.release()
    host = {"b_cfhd_getthumbnail_1_thread": [], "b_cfhd_getthumbnail_16_threads": []}
    for r in range(repeats):
        host["b_cfhd_getthumbnail_1_thread"].append(host_loop(L, samples, 1, window))
        host["b_cfhd_getthumbnail_16_threads"].append(host_loop(L, samples, 16, window))
    fps.update(host)
    med = {k: float(np.median(v)) for k, v in fps.items()}
    a = med["a_decode_queue_yuy2_from_hbm_%d_batches" % depth]
    result["queue"] = {"what": "per second: %d samples a pass; %d runs of %d s per variant, in turn" % (n, repeats, window), "per_second": {k: stats(v, 1) for k, v in fps.items()},
                       "thumbnails_from_hbm_over_a": round(med["thumbnails_from_hbm_%d_batches" % depth] / a, 2) if a > 0 else None}
    del owner
    if ctx: ctx.__exit__(None, None, None)
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
