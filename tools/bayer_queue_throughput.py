#!/usr/bin/env python3
"""Throughput of Bayer samples on the decode queue (cfhd_amd_decode_batch_create_bayer) and the time of its last level, the fused k_inv_bayer_strip against the pair
k_inv_packed16 + k_bayer_to_byr4: 3840 x 2160 BYR4 at FILMSCAN1 (the bench's Bayer geometry), 32 distinct mosaics encoded once by the product, the samples resident in
HBM (cfhd_amd_decode_batch_submit_device), the pictures left in HBM.  A run is sized by TIME (rounds of passes until `window` seconds have passed).
  capability   pictures per second of the queue (`large` samples a pass, `depth` batches in flight, the default route) against ONE CFHD_DecodeSample handle over the
               same samples, run after run in turn in the same process.  The handle is the one of the library CFHD_AMD_LIB names (another build: the parent commit's),
               else this library's own -- a handle never runs the fused kernel, so both are the route as it was.
  kernel       the HIP-event time of slot 6 (the last level with what follows it) on one batch alone, CFHD_AMD_INVERSE=tile and =strip alternated pass by pass,
               `passes` passes each: median and min .. max, for a small batch (`small` samples -- a 4K mosaic is 1920 x 1080 quads, one 1080p frame's worth: the
               fused route is the default from 4 on) and for the large one; the bytes each route reads and writes per pass, computed from the shapes, and the rate they give.
`emulated` as the last argument rehearses the whole tool on the CPU (cfhd_testlib.emulated_product) at 192 x 96 with 2 / 8 samples: the numbers mean nothing there.
The run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end, also written to `out` when given.
  python tools/bayer_queue_throughput.py [large=32] [small=4] [depth=2] [window=2] [repeats=3] [passes=9] [limit=500] [out] [emulated]"""
import ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_LIB = os.environ.pop("CFHD_AMD_LIB", None)        # (taken out before cfhd_testlib reads it: the queue under test is this tree's library)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import decode_queue as DQ
import bayer_queue as BQ

V = ctypes.c_void_p


def stats(values, digits=4):
    return {"median": round(float(np.median(values)), digits), "min": round(float(min(values)), digits), "max": round(float(max(values)), digits), "n": len(values)}


def timed(step, seconds):
    done = 0; t0 = time.perf_counter()
    while True:
        done += step()
        el = time.perf_counter() - t0
        if el >= seconds: return done / el


def main():
    emulated = sys.argv[-1] == "emulated"
    args = [a for a in sys.argv[1:] if a != "emulated"]
    arg = lambda k, d: int(args[k]) if len(args) > k and args[k] != "-" else d
    large, small, depth, window, repeats, passes, limit = arg(0, 32), arg(1, 4), arg(2, 2), arg(3, 2), arg(4, 3), arg(5, 9), arg(6, 500)
    out_path = args[7] if len(args) > 7 and args[7] != "-" else None
    signal.alarm(limit)                                   # the default action ends the process
    W, H, distinct = (3840, 2160, 32) if not emulated else (192, 96, 4)
    if emulated: large, small, window = min(large, 8), min(small, 2), 0
    ctx = T.emulated_product() if emulated else None
    if ctx: ctx.__enter__()
    L = BQ.lib()
    mosaics = [T.synth_bayer(W, H, 40 + i).reshape(-1).view(np.uint8).copy() for i in range(distinct)]
    unique = T.amd_encode_frames(mosaics, W * 2, W, H, BQ.BYR4, T.ENCODED_BAYER)
    del mosaics
    result = {"geometry": "%dx%d BYR4 FILMSCAN1, %d distinct samples in HBM" % (W, H, len(unique)), "sample_bytes_mean": int(np.mean([len(s) for s in unique])),
              "yardstick_library": ("another build named by CFHD_AMD_LIB: " + os.path.basename(YARDSTICK_LIB)) if YARDSTICK_LIB else "this library's own handle", "emulated": emulated}

    def passes_of(n):
        samples = [unique[i % len(unique)] for i in range(n)]
        blob, offsets, sizes = DQ.pack(samples)
        owner, dptr = DQ.device_copy(blob)
        return owner, (dptr if dptr is not None else owner.ptr), blob.nbytes, DQ._sizes(offsets), DQ._sizes(sizes)

    def run_pass(q, src, n):
        owner, dptr, nbytes, c_off, c_size = src
        assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, nbytes, c_off, c_size, n) == 0, T.amd_last_error()

    # ---- the kernel: slot 6 under tile and under strip, alternated pass by pass, one batch alone
    # bytes per pass from the shapes: the level-1 bands of four planes (rows of `pitch` coefficients, the row padding is not read), the scratch frame of four words per
    # quad (the pair only: written, then read), the mosaic
    bw, bh = W // 4, ((H // 2 + 7) // 8 * 8) // 2          # the level-1 band of a component plane (coded height)
    coeff = 4 * 4 * bw * bh * 2
    quads = (W // 2) * (H // 2)
    bytes_of = {"strip": {"read": coeff, "written": 8 * quads}, "tile": {"read": coeff + 8 * quads, "written": 8 * quads + 8 * quads}}
    result["kernel"] = {"what": "slot 6 of one batch alone (HIP events), CFHD_AMD_INVERSE=tile and =strip alternated pass by pass, %d passes each: ms median (min .. max); bytes per pass from the shapes" % passes}
    for label, n in (("small", small), ("large", large)):
        src = passes_of(n)
        q = BQ.Queue(unique[0], n)
        ms = {"tile": [], "strip": []}; names = {}; pictures = {}
        for mode in ("tile", "strip"):                      # warm-up
            with BQ.inverse(mode):
                run_pass(q, src, n); assert L.cfhd_amd_decode_batch_wait(q.b, None) == n, T.amd_last_error()
                pictures[mode] = q.pictures(min(n, 2)) + q.pictures(n)[-1:]      # (the first two and the last picture of the pass, at the size that is timed)
        assert all(np.array_equal(a, b) for a, b in zip(pictures["tile"], pictures["strip"])), "the fused kernel's pictures differ from the pair's"
        for _ in range(passes):
            for mode in ("tile", "strip"):
                with BQ.inverse(mode):
                    run_pass(q, src, n); assert L.cfhd_amd_decode_batch_wait(q.b, None) == n, T.amd_last_error()
                    ms[mode].append(float(L.cfhd_amd_decode_batch_kernel_ms(q.b, 6))); names[mode] = L.cfhd_amd_decode_batch_kernel_name(q.b, 6).decode()
        default_name = L.cfhd_amd_decode_batch_kernel_name(q.b, 6).decode()       # (no override: what the library's own rule picks for this batch)
        leg = {"samples": n, "frames_1080p_equivalent": round(n * (W // 2) * ((H // 2 + 7) // 8 * 8) / (1920.0 * 1080.0), 2), "default_route": default_name}
        for mode in ("tile", "strip"):
            med = float(np.median(ms[mode])); moved = n * (bytes_of[mode]["read"] + bytes_of[mode]["written"])
            leg[mode] = {"kernel": names[mode], "ms": stats(ms[mode]), "bytes_read": n * bytes_of[mode]["read"], "bytes_written": n * bytes_of[mode]["written"],
                         "gb_per_s": round(moved / (med * 1e-3) / 1e9, 1) if med > 0 else None}
        t, s = leg["tile"]["ms"], leg["strip"]["ms"]
        leg["pictures_equal"] = True                      # (asserted above: byte for byte, both routes)
        leg["strip_wins_beyond_the_spread"] = bool(s["max"] < t["min"])
        leg["tile_wins_beyond_the_spread"] = bool(t["max"] < s["min"])
        result["kernel"][label] = leg
        print(label, json.dumps(leg), flush=True)
        q.close(); del src

    # ---- the capability: the queue (default route) against one CFHD_DecodeSample handle, in turn
    src = passes_of(large)
    queues = [BQ.Queue(unique[0], large) for _ in range(depth)]
    def queue_round():
        for q in queues: run_pass(q, src, large)
        for q in queues: assert L.cfhd_amd_decode_batch_wait(q.b, None) == large, T.amd_last_error()
        return depth * large
    if YARDSTICK_LIB and not emulated:
        Y = ctypes.CDLL(YARDSTICK_LIB); T.declare_cfhd_api(Y)
    else: Y = L
    dec = V(); assert Y.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    sbs = [ctypes.create_string_buffer(s, len(s)) for s in unique]
    aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
    assert Y.CFHD_PrepareToDecode(dec, 0, 0, BQ.BYR4, 1, 0, sbs[0], len(unique[0]), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
    assert (aw.value, ah.value) == (W, H)
    plain = np.zeros(W * 2 * H, np.uint8)
    def handle_calls():
        for i in range(8): assert Y.CFHD_DecodeSample(dec, sbs[i % len(sbs)], len(unique[i % len(sbs)]), plain.ctypes.data_as(V), W * 2) == 0
        return 8
    queue_round(); handle_calls()                          # warm-up
    # the handle's picture of sample 7 (the last call of the warm-up) is the queue's, byte for byte
    assert np.array_equal(queues[0].pictures(8)[7], plain), "the queue's picture differs from the handle's"
    fps = {"queue": [], "handle": []}
    for r in range(repeats):
        fps["queue"].append(timed(queue_round, window)); fps["handle"].append(timed(handle_calls, window))
        print("repeat", r, {k: round(v[-1], 1) for k, v in fps.items()}, flush=True)
    result["capability"] = {"what": "pictures per second: %d samples a pass, %d batches in flight, the default route (%s), against one CFHD_DecodeSample handle (plain host memory); %d runs of %d s in turn" % (
                                large, depth, L.cfhd_amd_decode_batch_kernel_name(queues[0].b, 6).decode(), repeats, window),
                            "queue_fps": stats(fps["queue"], 1), "handle_fps": stats(fps["handle"], 1)}
    for q in queues: q.close()
    Y.CFHD_CloseDecoder(dec)
    del src
    if ctx: ctx.__exit__(None, None, None)
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
