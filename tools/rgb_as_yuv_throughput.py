#!/usr/bin/env python3
"""RGB 4:4:4 samples delivered as the reference's YU64 picture (CFHD_AMD_PICTURES_RGB_AS_YU64 / _RGB_AS_YUV422_U16 / _F16 / _F32): the time of k_dec_deliver_rgb_as_yuv
and what the decode queue makes of it, at 1920 x 1080, FILMSCAN1 RGB 4:4:4 samples (32 distinct frames encoded once by the product), output RG48, the samples resident
in HBM (cfhd_amd_decode_batch_submit_device), `n` samples a pass.  The method is tools/rgba_planes_throughput.py's; the yardstick is existing code measured in the same
call, never the new kernel's own numbers:
  deliver   cfhd_amd_decode_batch_kernel_ms index 9 on ONE batch alone, the variants alternated pass by pass, `passes` passes each: PACKED (k_dec_deliver: a straight
            copy of the RG48 pictures), PACKED a second time -- the run-to-run spread --, PLANAR_U16 / _F16 / _F32 (k_dec_deliver: R, G, B planes of the same
            pictures), then the four new layouts.  RGB_AS_YU64 and RGB_AS_YUV422_U16 / _F16 read 6 and write 4 bytes a pixel against 6 + 6 for PLANAR_U16.
  queue     pictures per second of the decode queue, `depth` batches in flight, delivery off / PLANAR_U16 / the four new layouts, run after run in turn, runs sized by
            TIME (`window` seconds), `repeats` runs each.
Medians with min .. max.  The run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end, also written to `out` when given.
`emulated` as the last argument rehearses the whole tool on the CPU (cfhd_testlib.emulated_product) at 192 x 96 with 8 samples: the numbers mean nothing there.
  python tools/rgb_as_yuv_throughput.py [n=256] [depth=2] [window=2] [repeats=3] [passes=9] [limit=900] [out] [emulated]"""
import ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import decode_queue as DQ
import gop_input_frames
import rgb_as_yuv as RY
from planar_frames_throughput import Hbm
from yuv422_planes_throughput import stats, timed

OFF, PACKED, PLANAR_U16, PLANAR_F16, PLANAR_F32 = -1, 0, 1, 2, 3
NAMES = {OFF: "no_delivery", PACKED: "packed", PLANAR_U16: "planar_u16", PLANAR_F16: "planar_f16", PLANAR_F32: "planar_f32",
         RY.RGB_AS_YU64: "rgb_as_yu64", RY.RGB_AS_YUV422_U16: "rgb_as_yuv422_u16", RY.RGB_AS_YUV422_F16: "rgb_as_yuv422_f16", RY.RGB_AS_YUV422_F32: "rgb_as_yuv422_f32"}
NEW = b"k_dec_deliver_rgb_as_yuv"


def measure(L, hbm, W, H, n, depth, window, repeats, passes, dptr, blob, c_off, c_size, first):
    picture_bytes = 6 * W * H
    result = {"picture_bytes": picture_bytes, "samples_a_pass": n}

    def geometry(layout):
        """(stride, pitch) of the contiguous picture of a layout."""
        if layout == PACKED: return picture_bytes, 6 * W
        if layout in (PLANAR_U16, PLANAR_F16, PLANAR_F32): row = W * (4 if layout == PLANAR_F32 else 2); return 3 * H * row, row
        if layout == RY.RGB_AS_YU64: return 4 * W * H, 4 * W
        row = W * RY.ELEMENT[layout]
        return 2 * H * row, row

    def moved(layout): return picture_bytes + geometry(layout)[0]      # bytes read + written per picture
    def is_new(layout): return layout >= RY.RGB_AS_YU64

    def set_delivery(q, target, layout):
        if layout == OFF: rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0)
        else: rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, target, geometry(layout)[0], geometry(layout)[1], layout)
        assert rc == 0, T.amd_last_error()

    def submit(q): assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, c_off, c_size, n) == 0, T.amd_last_error()
    def wait(q): assert L.cfhd_amd_decode_batch_wait(q.b, None) == n, T.amd_last_error()

    queues = [DQ.Queue(first, "RG48", DQ.FULL, n) for _ in range(depth)]
    tensors = [hbm.alloc(n * geometry(PLANAR_F32)[0]) for _ in range(depth)]      # (large enough for every layout)

    # ---- deliver: index 9 of one batch alone, the variants alternated pass by pass
    variants = [("packed", PACKED), ("packed_again", PACKED)] + [(NAMES[l], l) for l in (PLANAR_U16, PLANAR_F16, PLANAR_F32) + RY.LAYOUTS]
    ms = {name: [] for name, _ in variants}
    q = queues[0]
    for r in range(passes + 1):                               # (round 0: warm-up of every shape)
        for name, layout in variants:
            set_delivery(q, tensors[0], layout); submit(q); wait(q)
            assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == (NEW if is_new(layout) else b"k_dec_deliver")
            if r: ms[name].append(float(L.cfhd_amd_decode_batch_kernel_ms(q.b, 9)))
    deliver = {"what": "cfhd_amd_decode_batch_kernel_ms index 9, one batch alone, variants alternated pass by pass, %d passes each: ms per %d pictures, median (min .. max); "
                       "TB/s = bytes read + written per pass over the median; ratio = median over PLANAR_U16's" % (passes, n)}
    base = float(np.median(ms["planar_u16"]))
    for name, layout in variants:
        med = float(np.median(ms[name]))
        deliver[name] = {"kernel": NEW.decode() if is_new(layout) else "k_dec_deliver", "ms": stats(ms[name]), "bytes_moved_per_pass": n * moved(layout),
                         "tb_per_s": round(n * moved(layout) / (med * 1e-3) / 1e12, 3) if med > 0 else None, "ratio_to_planar_u16": round(med / base, 3) if base > 0 else None}
    both = ms["packed"] + ms["packed_again"]
    deliver["packed_spread_ms"] = {"min": round(min(both), 4), "max": round(max(both), 4), "medians": [deliver["packed"]["ms"]["median"], deliver["packed_again"]["ms"]["median"]]}
    result["deliver"] = deliver
    print("deliver", json.dumps(deliver), flush=True)

    # ---- queue: pictures per second, depth batches in flight, run after run in turn
    legs = [OFF, PLANAR_U16] + list(RY.LAYOUTS)
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
        if r: print("repeat", r, {k: round(v[-1], 1) for k, v in fps.items()}, flush=True)
    result["queue"] = {"what": "pictures per second of the decode queue: %d samples a pass, %d batches in flight; %d runs of %d s per variant, in turn" % (n, depth, repeats, window),
                       "fps": {k: stats(v, 1) for k, v in fps.items()}}
    for k in queues: k.close()
    hbm.release()
    return result


def main():
    emulated = sys.argv[-1] == "emulated"
    args = [a for a in sys.argv[1:] if a != "emulated"]
    arg = lambda k, d: int(args[k]) if len(args) > k and args[k] != "-" else d
    n, depth, window, repeats, passes, limit = arg(0, 256), arg(1, 2), arg(2, 2), arg(3, 3), arg(4, 9), arg(5, 900)
    out_path = args[6] if len(args) > 6 and args[6] != "-" else None
    signal.alarm(limit)                                   # the default action ends the process
    W, H, distinct = (1920, 1080, 32) if not emulated else (192, 96, 4)
    if emulated: n, window, passes = min(n, 8), 0, min(passes, 2)
    ctx = T.emulated_product() if emulated else None
    if ctx: ctx.__enter__()
    L = RY.lib()
    frames, pitch = gop_input_frames.frames("RG48", W, H, distinct)
    unique = T.amd_encode_frames([np.ascontiguousarray(f) for f in frames], pitch, W, H, T.PIX_RG48, T.ENCODED_RGB444, T.QUALITY_FILMSCAN1, 0)
    result = {"geometry": "%dx%d RGB 4:4:4 FILMSCAN1 samples (%d distinct), output RG48, samples in HBM" % (W, H, len(unique)), "emulated": emulated}
    samples = [unique[i % len(unique)] for i in range(n)]
    blob, offsets, sizes = DQ.pack(samples)
    owner, dptr = DQ.device_copy(blob)
    if dptr is None: dptr = owner.ptr
    result["rg48"] = measure(L, Hbm(emulated), W, H, n, depth, window, repeats, passes, dptr, blob, DQ._sizes(offsets), DQ._sizes(sizes), unique[0])
    del owner
    if ctx: ctx.__exit__(None, None, None)
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
