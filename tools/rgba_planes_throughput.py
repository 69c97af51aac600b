#!/usr/bin/env python3
"""Pictures that carry alpha (b64a, BGRA) as planar R, G, B, A tensors in HBM, both ways: the times of k_dec_deliver_rgba and k_enc_collect_rgba and what the decode
queue makes of them, at 1920 x 1080, FILMSCAN1 4:2:2 samples (32 distinct frames encoded once by the product), the samples resident in HBM
(cfhd_amd_decode_batch_submit_device).  Once for a b64a batch of `n16` samples a pass (U16 / F16 / F32) and once for a BGRA batch of `n8` (U8 / F16 / F32; bottom row
first in its packed form, the flip is part of what is measured).  The method is tools/yuv422_planes_throughput.py's; the yardstick is existing code measured in the
same call, never the new kernels' own numbers:
  deliver   cfhd_amd_decode_batch_kernel_ms index 9 on ONE batch alone, the variants alternated pass by pass, `passes` passes each: PACKED (k_dec_deliver: a straight
            copy of the same pictures), PACKED a second time -- the run-to-run spread of the yardstick --, then the three plane layouts of the format.  The native
            layout (U8 / U16) and, for b64a, F16 move exactly the packed copy's bytes.
  collect   an encode-only batch of `nc` = min(n, 256) frames of the format: cfhd_amd_batch_kernel_ms index 20 of ONE cfhd_amd_batch_upload_device_planar call per
            layout, and the wall time (device idle before, hipDeviceSynchronize behind) of that call against `nc` cfhd_amd_batch_upload_device copies, alternated.
  queue     pictures per second of the decode queue, `depth` batches in flight, delivery off / PACKED / the three plane layouts, run after run in turn, runs sized by
            TIME (`window` seconds), `repeats` runs each.
Medians with min .. max.  The run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end, also written to `out` when given.
`emulated` as the last argument rehearses the whole tool on the CPU (cfhd_testlib.emulated_product) at 192 x 96 with 8 samples: the numbers mean nothing there.
  python tools/rgba_planes_throughput.py [n16=128] [n8=512] [depth=2] [window=2] [repeats=3] [passes=9] [limit=900] [out] [emulated]"""
import ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import decode_queue as DQ
import rgba_planes as RP
from planar_frames_throughput import Hbm
from yuv422_planes_throughput import stats, timed

V = ctypes.c_void_p
OFF, PACKED = -1, 0
NAMES = {OFF: "no_delivery", PACKED: "packed", RP.RGBA_U8: "rgba_u8", RP.RGBA_U16: "rgba_u16", RP.RGBA_F16: "rgba_f16", RP.RGBA_F32: "rgba_f32"}


def measure(L, hbm, fmt, W, H, n, depth, window, repeats, passes, dptr, blob, c_off, c_size, first):
    picture_bytes = RP.row_bytes(fmt, W) * H
    layouts = RP.layouts_of(fmt)
    result = {"picture_bytes": picture_bytes, "samples_a_pass": n}

    def geometry(layout):
        """(stride, pitch) of the contiguous picture of a layout."""
        if layout == PACKED: return picture_bytes, RP.row_bytes(fmt, W)
        row = W * RP.ELEMENT[layout]
        return 4 * H * row, row

    def moved(layout): return picture_bytes + geometry(layout)[0]      # bytes read + written per picture

    def set_delivery(q, target, layout):
        if layout == OFF: rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0)
        else: rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, target, geometry(layout)[0], geometry(layout)[1], layout)
        assert rc == 0, T.amd_last_error()

    def submit(q): assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, c_off, c_size, n) == 0, T.amd_last_error()
    def wait(q): assert L.cfhd_amd_decode_batch_wait(q.b, None) == n, T.amd_last_error()

    queues = [DQ.Queue(first, fmt, DQ.FULL, n) for _ in range(depth)]
    tensors = [hbm.alloc(n * geometry(RP.RGBA_F32)[0]) for _ in range(depth)]      # (large enough for every layout)

    # ---- deliver: index 9 of one batch alone, the variants alternated pass by pass
    variants = [("packed", PACKED), ("packed_again", PACKED)] + [(NAMES[l], l) for l in layouts]
    ms = {name: [] for name, _ in variants}
    q = queues[0]
    for r in range(passes + 1):                               # (round 0: warm-up of every shape)
        for name, layout in variants:
            set_delivery(q, tensors[0], layout); submit(q); wait(q)
            assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == (b"k_dec_deliver" if layout == PACKED else RP.DELIVER)
            if r: ms[name].append(float(L.cfhd_amd_decode_batch_kernel_ms(q.b, 9)))
    deliver = {"what": "cfhd_amd_decode_batch_kernel_ms index 9, one batch alone, variants alternated pass by pass, %d passes each: ms per %d pictures, median (min .. max); "
                       "TB/s = bytes read + written per pass over the median; ratio = median over the packed copy's" % (passes, n)}
    base = float(np.median(ms["packed"] + ms["packed_again"]))
    for name, layout in variants:
        med = float(np.median(ms[name]))
        deliver[name] = {"kernel": "k_dec_deliver" if layout == PACKED else "k_dec_deliver_rgba", "ms": stats(ms[name]), "bytes_moved_per_pass": n * moved(layout),
                         "tb_per_s": round(n * moved(layout) / (med * 1e-3) / 1e12, 3) if med > 0 else None, "ratio_to_packed": round(med / base, 3) if base > 0 else None}
    both = ms["packed"] + ms["packed_again"]
    deliver["packed_spread_ms"] = {"min": round(min(both), 4), "max": round(max(both), 4), "medians": [deliver["packed"]["ms"]["median"], deliver["packed_again"]["ms"]["median"]]}
    result["deliver"] = deliver
    print(fmt, "deliver", json.dumps(deliver), flush=True)

    # ---- collect: an encode-only batch fed from the planes the queue just delivered, against upload_device copies of the packed pictures
    nc = min(n, 256)
    packed = hbm.alloc(n * picture_bytes)
    set_delivery(q, packed, PACKED); submit(q); wait(q)
    b = L.cfhd_amd_batch_create_ex(W, H, RP.PIX[fmt], T.ENCODED_YUV422, 0, T.QUALITY_FILMSCAN1, nc, 1, 1)
    assert b, T.amd_last_error()
    assert L.cfhd_amd_batch_kernel_name(b, 20) == RP.COLLECT
    sync = hbm.hip.hipDeviceSynchronize if hbm.hip is not None else (lambda: 0)
    planes = {layout: hbm.alloc(n * geometry(layout)[0]) for layout in layouts}
    for layout, mem in planes.items(): set_delivery(q, mem, layout); submit(q); wait(q)
    set_delivery(q, None, OFF)

    def feed(layout):
        """Wall ms of feeding the batch's nc frames, device idle before and after."""
        assert sync() == 0
        t0 = time.perf_counter()
        if layout == PACKED:
            for i in range(nc): assert L.cfhd_amd_batch_upload_device(b, i, packed + i * picture_bytes, RP.row_bytes(fmt, W)) == 0, T.amd_last_error()
        else: assert L.cfhd_amd_batch_upload_device_planar(b, 0, nc, planes[layout], geometry(layout)[0], geometry(layout)[1], layout) == 0, T.amd_last_error()
        assert sync() == 0
        return (time.perf_counter() - t0) * 1e3

    cvariants = [("upload_device", PACKED), ("upload_device_again", PACKED)] + [(NAMES[l], l) for l in layouts]
    wall = {name: [] for name, _ in cvariants}; kernel = {name: [] for name, _ in cvariants}; sample_bytes = {}
    for r in range(passes + 1):
        for name, layout in cvariants:
            w_ms = feed(layout)
            total = L.cfhd_amd_batch_roundtrip(b)
            assert total > 0, (total, T.amd_last_error())
            sample_bytes.setdefault(name, int(total))
            if r: wall[name].append(w_ms); kernel[name].append(float(L.cfhd_amd_batch_kernel_ms(b, 20)))
    # (the native layout and F32 give back the packed frame: the same samples as the copies')
    assert sample_bytes["upload_device"] == sample_bytes[NAMES[layouts[0]]] == sample_bytes["rgba_f32"], sample_bytes
    collect = {"what": "one encode-only batch of %d frames, variants alternated, %d rounds: wall ms of feeding all frames (device idle before, hipDeviceSynchronize behind) and "
                       "cfhd_amd_batch_kernel_ms index 20 (0 for the copies, which run no kernel of the library); TB/s from the kernel's median" % (nc, passes), "sample_bytes_per_pass": sample_bytes}
    for name, layout in cvariants:
        leg = {"wall_ms": stats(wall[name]), "bytes_moved_per_pass": nc * moved(layout)}
        if layout != PACKED:
            med = float(np.median(kernel[name]))
            leg["k_enc_collect_rgba_ms"] = stats(kernel[name]); leg["tb_per_s"] = round(nc * moved(layout) / (med * 1e-3) / 1e12, 3) if med > 0 else None
        else: assert not any(kernel[name]), "a pass fed by upload_device has no collect time"
        collect[name] = leg
    result["collect"] = collect
    print(fmt, "collect", json.dumps(collect), flush=True)
    L.cfhd_amd_batch_destroy(b)

    # ---- queue: pictures per second, depth batches in flight, run after run in turn
    legs = [OFF, PACKED] + layouts
    def queue_round():
        for k in queues: submit(k)
        for k in queues: wait(k)
        return depth * n
    fps = {NAMES[leg]: [] for leg in legs}
    for r in range(repeats + 1):                              # (round 0: warm-up, not recorded)
        for leg in legs:
            for k, qq in enumerate(queues): set_delivery(qq, tensors[k], leg)
            v = timed(queue_round, window if r else 0)
            if r: fps[NAMES[leg]].append(v)
        if r: print(fmt, "repeat", r, {k: round(v[-1], 1) for k, v in fps.items()}, flush=True)
    result["queue"] = {"what": "pictures per second of the decode queue: %d samples a pass, %d batches in flight; %d runs of %d s per variant, in turn" % (n, depth, repeats, window),
                       "fps": {k: stats(v, 1) for k, v in fps.items()}}
    for k in queues: k.close()
    hbm.release()
    return result


def main():
    emulated = sys.argv[-1] == "emulated"
    args = [a for a in sys.argv[1:] if a != "emulated"]
    arg = lambda k, d: int(args[k]) if len(args) > k and args[k] != "-" else d
    n16, n8, depth, window, repeats, passes, limit = arg(0, 128), arg(1, 512), arg(2, 2), arg(3, 2), arg(4, 3), arg(5, 9), arg(6, 900)
    out_path = args[7] if len(args) > 7 and args[7] != "-" else None
    signal.alarm(limit)                                   # the default action ends the process
    W, H, distinct = (1920, 1080, 32) if not emulated else (192, 96, 4)
    if emulated: n16, n8, window, passes = min(n16, 8), min(n8, 8), 0, min(passes, 2)
    ctx = T.emulated_product() if emulated else None
    if ctx: ctx.__enter__()
    L = RP.lib()
    frames = [np.ascontiguousarray(T.synth_yuy2(W, H, 40 + i)[0]) for i in range(distinct)]
    unique = T.amd_encode_frames(frames, W * 2, W, H)
    del frames
    result = {"geometry": "%dx%d 4:2:2 FILMSCAN1 samples (%d distinct), samples in HBM" % (W, H, len(unique)), "emulated": emulated}
    for fmt, n in (("b64a", n16), ("BGRA", n8)):
        samples = [unique[i % len(unique)] for i in range(n)]
        blob, offsets, sizes = DQ.pack(samples)
        owner, dptr = DQ.device_copy(blob)
        if dptr is None: dptr = owner.ptr
        result[fmt] = measure(L, Hbm(emulated), fmt, W, H, n, depth, window, repeats, passes, dptr, blob, DQ._sizes(offsets), DQ._sizes(sizes), unique[0])
        del owner
    if ctx: ctx.__exit__(None, None, None)
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
