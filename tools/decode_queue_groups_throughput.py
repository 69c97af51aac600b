#!/usr/bin/env python3
"""Throughput of the decode queue over a stream of two-frame groups (cfhd_amd_decode_batch_create_groups): 1920 x 1080, 32 distinct frames = 16 groups encoded once by
the product at FILMSCAN1 from YUY2, decoded to YUY2: `groups` groups a pass (2 * groups samples and pictures), `depth` batches in flight (submit all, wait in order),
warmed up; a run is sized by TIME as in tools/decode_queue_throughput.py, run after run in turn (`repeats` times each), all in one process:
  (a) host_to_host   the samples in a registered host blob, the pictures to registered host memory,
  (b) device         the blob already in HBM (cfhd_amd_decode_batch_submit_device), the pictures left in HBM,
  (c) c_abi_sync     one CFHD_DecodeSample handle over the same stream, plain host memory: group, P-frame sample, group, ...
Then (b) and (c) again for a stream from RG24 input (subband 7 coded in two passes: k_dec_band_two_pass on the queue, the host coder on the handle).  Every figure is
pictures per second over a run; mean and spread (min .. max) over the runs.  Also the HIP-event time of every kernel slot (8: k_dec_band_two_pass alone) over
`kernel_passes` passes of (a) on ONE batch with nothing else in flight, for both streams.  The whole run ends itself after `limit` seconds (SIGALRM) rather than hang.
One JSON line at the end, also written to `out` when given.
  python tools/decode_queue_groups_throughput.py [groups=256] [depth=4] [window=3] [repeats=3] [limit=500] [out] [kernel_passes=9]"""
import ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import decode_queue as DQ
import group_decode_queue as GQ

W, H = 1920, 1080
V = ctypes.c_void_p


def spread(runs):
    fps = [f for f, _ in runs]
    return {"mean": round(float(np.mean(fps)), 1), "min": round(float(min(fps)), 1), "max": round(float(max(fps)), 1), "runs": len(fps), "window_seconds": [round(t, 2) for _, t in runs]}


def timed(step, seconds):
    """(units per second, seconds) of step() -- which returns the units it did -- repeated until `seconds` have passed."""
    done = 0; t0 = time.perf_counter()
    while True:
        done += step()
        el = time.perf_counter() - t0
        if el >= seconds: return done / el, el


def measure(L, pix, frames, pitch, ng, depth, window, repeats, kernel_passes, variants):
    """The figures of one stream: its 32 frames encoded as 16 groups, the pass made of them in turn."""
    stream = T.amd_encode_frames(frames + [frames[0]], pitch, W, H, GQ.FOURCCS[pix], T.ENCODED_YUV422, T.QUALITY_FILMSCAN1, GQ.GOP)
    assert len(stream) == len(frames) + 1 and len(stream[0]) == 40
    unique = stream[1:]
    n = 2 * ng
    samples = [unique[i % len(unique)] for i in range(n)]
    blob, offsets, sizes = DQ.pack(samples)
    fbytes = W * 2 * H
    register = lambda a: L.cfhd_amd_register_host_buffer(a.ctypes.data_as(V), a.nbytes)
    assert register(blob) == 0
    dsts = [np.zeros(n * fbytes, np.uint8) for _ in range(depth)] if "host_to_host" in variants else []
    for d in dsts: assert register(d) == 0
    owner, dptr = DQ.device_copy(blob)
    if dptr is None: dptr = owner.ptr
    queues = [GQ.GroupQueue(samples[0], "YUY2", DQ.FULL, ng) for _ in range(depth)]
    c_off, c_size = DQ._sizes(offsets), DQ._sizes(sizes)
    out = {"source": "%dx%d %s FILMSCAN1, %d distinct frames = %d groups" % (W, H, pix, len(frames), len(frames) // 2), "group_sample_bytes_mean": int(np.mean(sizes[0::2]))}

    def decode_run(variant, seconds, use=None):
        use = use if use is not None else range(depth)
        def submit(k):
            q = queues[k]
            if variant == "device": rc = L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, c_off, c_size, n)
            else: rc = L.cfhd_amd_decode_batch_submit_host(q.b, blob.ctypes.data_as(V), c_off, c_size, n, dsts[k].ctypes.data_as(V) if dsts else None, fbytes, W * 2)
            assert rc == 0, (rc, T.amd_last_error())
        def one_round():
            for k in use: submit(k)
            for k in use: assert L.cfhd_amd_decode_batch_wait(queues[k].b, None) == n, T.amd_last_error()
            return len(use) * n
        return timed(one_round, seconds)

    dec = V(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    sbs = [ctypes.create_string_buffer(s, len(s)) for s in unique]
    aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
    assert L.CFHD_PrepareToDecode(dec, 0, 0, T.PIX_YUY2, 1, 0, sbs[0], len(unique[0]), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
    plain = np.zeros(fbytes, np.uint8)

    def c_abi_run(seconds):
        def calls():
            for i in range(len(sbs)): assert L.CFHD_DecodeSample(dec, sbs[i], len(unique[i]), plain.ctypes.data_as(V), W * 2) == 0
            return len(sbs)
        return timed(calls, seconds)

    for v in variants: decode_run(v, 0)                       # warm-up: every path once
    c_abi_run(0)
    fps = {k: [] for k in variants + ("c_abi_sync",)}
    for r in range(repeats):                                  # run after run in turn: what drifts, drifts for all
        for v in variants: fps[v].append(decode_run(v, window))
        fps["c_abi_sync"].append(c_abi_run(window))
        print(pix, "repeat", r, {k: (round(x[-1][0], 1), round(x[-1][1], 2)) for k, x in fps.items()}, flush=True)
    out["fps"] = {k: spread(x) for k, x in fps.items()}
    c = out["fps"]["c_abi_sync"]; margin = c["max"] - c["min"]
    out["claim"] = {"what": "every queue variant is not slower than one CFHD_DecodeSample handle over the same stream (c) measured beside it, within (c)'s own min-max spread",
                    "margin_fps": round(margin, 1), **{v + "_holds": bool(out["fps"][v]["mean"] >= c["mean"] - margin) for v in variants}}
    # the kernel slots: passes on one batch alone, nothing else in flight on the device
    q = queues[0]
    names = [L.cfhd_amd_decode_batch_kernel_name(q.b, k).decode() for k in range(8)] + ["k_dec_band_two_pass"]
    per_pass = []
    for _ in range(kernel_passes):
        decode_run(variants[0], 0, use=[0])
        per_pass.append([float(L.cfhd_amd_decode_batch_kernel_ms(q.b, k)) for k in range(9)])
    per_pass = np.array(per_pass)
    out["kernel_ms"] = {"what": "one batch alone, %d passes of %s: median (min .. max); 8 is part of 2" % (kernel_passes, variants[0]),
                        **{"%d %s" % (k, names[k]): {"median": round(float(np.median(per_pass[:, k])), 4), "min": round(float(per_pass[:, k].min()), 4), "max": round(float(per_pass[:, k].max()), 4)} for k in range(9)}}
    for q in queues: q.close()
    L.CFHD_CloseDecoder(dec)
    for a_ in [blob] + dsts: L.cfhd_amd_unregister_host_buffer(a_.ctypes.data_as(V))
    del owner
    return out


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    ng, depth, window, repeats, limit = arg(1, 256), arg(2, 4), arg(3, 3), arg(4, 3), arg(5, 500)
    kernel_passes = arg(7, 9)
    out_path = sys.argv[6] if len(sys.argv) > 6 else None
    signal.alarm(limit)                                   # the default action ends the process
    L = GQ.lib()
    frames, pitch = T.qbist_frames(10, 32, W, H, T.PIX_YUY2) if T.have_ref() else ([T.synth_yuy2(W, H, 70 + i)[0] for i in range(32)], W * 2)
    result = {"geometry": "%dx%d two-frame groups to YUY2" % (W, H), "groups_per_pass": ng, "pictures_per_pass": 2 * ng, "passes_in_flight": depth, "window_seconds_asked": window}
    result["yuy2_source"] = measure(L, "YUY2", [np.ascontiguousarray(f) for f in frames], pitch, ng, depth, window, repeats, kernel_passes, ("host_to_host", "device"))
    rgb, rgb_pitch = GQ._rgb8_frames("RG24", W, H, 32)
    result["rg24_source"] = measure(L, "RG24", rgb, rgb_pitch, ng, depth, window, repeats, kernel_passes, ("device",))
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
