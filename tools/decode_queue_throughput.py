#!/usr/bin/env python3
"""Throughput of the decode queue (cfhd_amd_decode_batch_*), 1920 x 1080 samples of 32 Qbist frames encoded once by the product at FILMSCAN1, decoded to YUY2:
`samples` samples a pass, `depth` decode batches in flight (submit all, wait in order), warmed up; a run is sized by TIME: rounds of depth passes (C-ABI: calls) until
`window` seconds have passed, whatever the variant's rate, and the JSON records how long every run lasted.
  (a) host_to_host   the samples in a registered host blob, the pictures to registered host memory (one DMA each way per pass),
  (b) host_to_hbm    the same blob, the pictures left in HBM,
  (c) device         the blob already in HBM (cfhd_amd_decode_batch_submit_device), the pictures left in HBM,
and, in the same process, run after run in turn (`repeats` times each):
  (d) c_abi_sync     one CFHD_DecodeSample handle over the same samples, plain host memory (tools/sync_api_rate.py's way),
  (e) round_trip     the unchanged frame queue fed from registered host memory, pictures back to registered memory (cfhd_amd_batch_submit_host: bench.py's host_fed),
                     the same frames a pass and the same passes in flight.
Every figure is frames per second over a run; mean and spread (min .. max) over the runs.  Also the HIP-event time of every kernel slot over `kernel_passes` passes of (a)
on ONE batch with nothing else in flight (median, min, max) and what k_dec_ingest moves in its median time (bytes read + bytes written).  The whole run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end,
also written to `out` when given.
The device-delivery leg (cfhd_amd_decode_batch_set_device_pictures; left out, "device_delivery": null, on a library without the entry point -- CFHD_AMD_LIB names another
build, so one tool measures both sides of a change): the samples in HBM as in (c), and per pass the pictures
  (f) left in HBM, as (c), for YUY2 and for RG48 batches,
  (g) delivered by k_dec_deliver into device memory of the caller's: PACKED YUY2, PACKED RG48, PLANAR_F16 of RG48 (contiguous (n, 3, H, W) tensors),
run after run in turn with (f) of the same output; k_dec_deliver's HIP-event time per pass on one batch alone and the bytes it reads and writes in that time.
`legs` = delivery runs (c) and this leg only.
  python tools/decode_queue_throughput.py [samples=512] [depth=4] [window=3] [repeats=3] [limit=500] [out] [kernel_passes=9] [legs=all]"""
import ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import decode_queue as DQ
import group_batches as GB

W, H = 1920, 1080
V = ctypes.c_void_p


def spread(runs):
    fps = [f for f, _ in runs]
    return {"mean": round(float(np.mean(fps)), 1), "min": round(float(min(fps)), 1), "max": round(float(max(fps)), 1), "runs": len(fps), "window_seconds": [round(t, 2) for _, t in runs]}


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    n, depth, window, repeats, limit = arg(1, 512), arg(2, 4), arg(3, 3), arg(4, 3), arg(5, 500)
    kernel_passes = arg(7, 9)
    out_path = sys.argv[6] if len(sys.argv) > 6 and sys.argv[6] != "-" else None
    legs = sys.argv[8] if len(sys.argv) > 8 else "all"
    signal.alarm(limit)                                   # the default action ends the process
    L = DQ.lib(); GB.lib()
    frames, pitch = T.qbist_frames(10, 32, W, H, T.PIX_YUY2) if T.have_ref() else ([T.synth_yuy2(W, H, 70 + i)[0] for i in range(32)], W * 2)
    unique = T.amd_encode_frames(frames, pitch, W, H)
    samples = [unique[i % len(unique)] for i in range(n)]
    blob, offsets, sizes = DQ.pack(samples)
    fbytes = pitch * H
    register = lambda a: L.cfhd_amd_register_host_buffer(a.ctypes.data_as(V), a.nbytes)
    assert register(blob) == 0
    host_legs = n if legs != "delivery" else 0                # (the host-memory legs' buffers: none where only the device legs run)
    dsts = [np.zeros(max(host_legs * fbytes, 16), np.uint8) for _ in range(depth)]
    for d in dsts: assert register(d) == 0
    src = np.empty(max(host_legs * fbytes, 16), np.uint8)
    for i in range(host_legs): src[i * fbytes:(i + 1) * fbytes] = frames[i % len(frames)][:fbytes]
    assert register(src) == 0
    owner, dptr = DQ.device_copy(blob)
    if dptr is None: dptr = owner.ptr
    queues = [DQ.Queue(samples[0], "YUY2", DQ.FULL, n) for _ in range(depth)]
    c_off, c_size = DQ._sizes(offsets), DQ._sizes(sizes)
    result = {"geometry": "%dx%d YUY2 FILMSCAN1, %d distinct samples" % (W, H, len(unique)), "samples_per_pass": n, "passes_in_flight": depth, "window_seconds_asked": window,
              "sample_bytes_mean": int(np.mean(sizes))}

    def timed(step, seconds):
        """(units per second, seconds) of step() -- which returns the units it did -- repeated until `seconds` have passed."""
        done = 0; t0 = time.perf_counter()
        while True:
            done += step()
            el = time.perf_counter() - t0
            if el >= seconds: return done / el, el

    def decode_run(variant, seconds, use=None, queues=queues):
        use = use if use is not None else range(depth)
        def submit(k):
            q = queues[k]
            if variant == "device": rc = L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, c_off, c_size, n)
            else: rc = L.cfhd_amd_decode_batch_submit_host(q.b, blob.ctypes.data_as(V), c_off, c_size, n, dsts[k].ctypes.data_as(V) if variant == "host_to_host" else None, fbytes, pitch)
            assert rc == 0, (rc, T.amd_last_error())
        def one_round():
            for k in use: submit(k)
            for k in use: assert L.cfhd_amd_decode_batch_wait(queues[k].b, None) == n, T.amd_last_error()
            return len(use) * n
        return timed(one_round, seconds)

    everything = legs != "delivery"
    batches = []
    for _ in range(depth if everything else 0):
        b = L.cfhd_amd_batch_create_ex(W, H, T.PIX_YUY2, T.ENCODED_YUV422, 0, T.QUALITY_FILMSCAN1, n, 1, 0)
        assert b, T.amd_last_error()
        batches.append(b)

    def round_trip_run(seconds):
        def one_round():
            for k in range(depth): assert L.cfhd_amd_batch_submit_host(batches[k], src.ctypes.data_as(V), fbytes, pitch, dsts[k].ctypes.data_as(V), fbytes, pitch) == 0, T.amd_last_error()
            for k in range(depth): assert L.cfhd_amd_batch_wait(batches[k]) > 0, T.amd_last_error()
            return depth * n
        return timed(one_round, seconds)

    dec = V(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    sbs = [ctypes.create_string_buffer(s, len(s)) for s in unique]
    aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
    assert L.CFHD_PrepareToDecode(dec, 0, 0, T.PIX_YUY2, 1, 0, sbs[0], 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
    plain = np.zeros(fbytes, np.uint8)

    def c_abi_run(seconds):
        def calls():
            for i in range(64): assert L.CFHD_DecodeSample(dec, sbs[i % len(sbs)], len(unique[i % len(sbs)]), plain.ctypes.data_as(V), pitch) == 0
            return 64
        return timed(calls, seconds)

    variants = ("host_to_host", "host_to_hbm", "device") if everything else ("device",)
    for v in variants: decode_run(v, 0)                       # warm-up: every path once
    if everything: round_trip_run(0); c_abi_run(0)
    fps = {k: [] for k in variants + (("c_abi_sync", "round_trip") if everything else ())}
    for r in range(repeats):                                  # run after run in turn: what drifts, drifts for all
        for v in variants: fps[v].append(decode_run(v, window))
        if everything:
            fps["c_abi_sync"].append(c_abi_run(window))
            fps["round_trip"].append(round_trip_run(window))
        print("repeat", r, {k: (round(x[-1][0], 1), round(x[-1][1], 2)) for k, x in fps.items()}, flush=True)
    result["fps"] = {k: spread(x) for k, x in fps.items()}
    if everything: kernel_slots(L, result, queues, decode_run, sizes, kernel_passes)
    result["device_delivery"] = device_delivery(L, queues, samples, decode_run, dptr, n, depth, window, repeats, kernel_passes)      # (closes the YUY2 batches)
    for b in batches: L.cfhd_amd_batch_destroy(b)
    L.CFHD_CloseDecoder(dec)
    for a_ in [blob, src] + dsts: L.cfhd_amd_unregister_host_buffer(a_.ctypes.data_as(V))
    del owner
    finish(result, out_path)


def kernel_slots(L, result, queues, decode_run, sizes, kernel_passes):
    # the kernel slots: passes of (a) on one batch alone, nothing else in flight on the device
    q = queues[0]
    names = [L.cfhd_amd_decode_batch_kernel_name(q.b, k).decode() for k in range(8)]
    per_pass = []
    for _ in range(kernel_passes):
        decode_run("host_to_host", 0, use=[0])
        per_pass.append([float(L.cfhd_amd_decode_batch_kernel_ms(q.b, k)) for k in range(8)])
    per_pass = np.array(per_pass)
    ms = [float(np.median(per_pass[:, k])) for k in range(8)]
    result["kernel_ms"] = {"what": "one batch alone, %d passes: median (min .. max)" % kernel_passes,
                           **{"%d %s" % (k, names[k]): {"median": round(ms[k], 4), "min": round(float(per_pass[:, k].min()), 4), "max": round(float(per_pass[:, k].max()), 4)} for k in range(8)}}
    moved = sum(sizes) + sum((s + 255) & ~255 for s in sizes)
    result["k_dec_ingest"] = {"ms_median": round(ms[0], 4), "bytes_read": int(sum(sizes)), "bytes_written": int(moved - sum(sizes)), "gb_per_s": round(moved / (ms[0] * 1e-3) / 1e9, 1) if ms[0] > 0 else None}
    rt, a = result["fps"]["round_trip"], result["fps"]["host_to_host"]
    result["claim"] = {"what": "the host-fed decode queue (a) is not slower than the host-fed round trip (e) measured beside it, within the round trip's own run-to-run spread",
                       "margin_fps": round(rt["max"] - rt["min"], 1), "holds": bool(a["mean"] >= rt["mean"] - (rt["max"] - rt["min"]))}


def finish(result, out_path):
    signal.alarm(0)
    line = json.dumps(result)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


def device_delivery(L, yuy2_queues, samples, decode_run, dptr, n, depth, window, repeats, kernel_passes):
    """The device-delivery leg: None on a library without cfhd_amd_decode_batch_set_device_pictures."""
    if not hasattr(L, "cfhd_amd_decode_batch_set_device_pictures"):
        for q in yuy2_queues: q.close()
        return None
    set_pictures = L.cfhd_amd_decode_batch_set_device_pictures
    set_pictures.argtypes = [V, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    hip = DQ.DeviceBlob(np.zeros(16, np.uint8)).hip           # (the runtime the library loaded, on the library's device)
    PACKED, PLANAR_F16 = 0, 2
    out = {"what": "samples in HBM (submit_device), %d a pass, %d passes in flight; fps: mean (min .. max) over %d runs of %d s, left_in_hbm and delivered in turn; k_dec_deliver: one batch alone, "
                   "HIP events, median over %d passes, bytes = pictures read + pictures written" % (n, depth, repeats, window, kernel_passes)}

    def leg(name, queues, layout, row_bytes, planes):
        q = queues[0]
        pitch = row_bytes; stride = planes * q.h * pitch
        buffers = []
        for _ in queues:
            p = V(); assert hip.hipMalloc(ctypes.byref(p), n * stride) == 0, "hipMalloc of %d bytes" % (n * stride)
            buffers.append(p)
        try:
            runs = {"left_in_hbm": [], "delivered": []}
            def switch(on):
                for q_, p in zip(queues, buffers): assert set_pictures(q_.b, p if on else None, stride, pitch, layout) == 0, T.amd_last_error()
            switch(True); decode_run("device", 0, queues=queues); switch(False); decode_run("device", 0, queues=queues)      # warm-up
            for r in range(repeats):
                switch(False); runs["left_in_hbm"].append(decode_run("device", window, queues=queues))
                switch(True); runs["delivered"].append(decode_run("device", window, queues=queues))
                print(name, "repeat", r, {k: round(x[-1][0], 1) for k, x in runs.items()}, flush=True)
            ms = []
            for _ in range(kernel_passes):
                decode_run("device", 0, use=[0], queues=queues)
                ms.append(float(L.cfhd_amd_decode_batch_kernel_ms(q.b, 9)))
            assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
            pass_ms = sum(float(L.cfhd_amd_decode_batch_kernel_ms(q.b, k)) for k in range(8))
            switch(False)
            med = float(np.median(ms)); moved = n * (q.row_bytes * q.h + planes * q.h * row_bytes)
            return {"fps": {k: spread(x) for k, x in runs.items()}, "picture_bytes_in": q.row_bytes * q.h, "picture_bytes_out": planes * q.h * row_bytes,
                    "k_dec_deliver_ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}, "kernel_slots_0_to_7_ms_last_pass": round(pass_ms, 4),
                    "bytes_moved_per_pass": int(moved), "gb_per_s": round(moved / (med * 1e-3) / 1e9, 1) if med > 0 else None}
        finally:
            for p in buffers: hip.hipFree(p)

    q = yuy2_queues[0]
    out["packed_yuy2"] = leg("packed_yuy2", yuy2_queues, PACKED, q.row_bytes, 1)
    for q in yuy2_queues: q.close()                           # (their pictures' HBM goes to the RG48 batches)
    rg48 = [DQ.Queue(samples[0], "RG48", DQ.FULL, n) for _ in range(depth)]
    try:
        out["packed_rg48"] = leg("packed_rg48", rg48, PACKED, rg48[0].row_bytes, 1)
        out["planar_f16"] = leg("planar_f16", rg48, PLANAR_F16, rg48[0].w * 2, 3)
    finally:
        for q in rg48: q.close()
    return out


if __name__ == "__main__":
    main()
