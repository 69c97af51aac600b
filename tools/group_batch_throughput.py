#!/usr/bin/env python3
"""Throughput of two-frame groups (CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP), 1920 x 1080 YUY2, FILMSCAN1, round trips of `frames` frames per pass:
  (a) one CFHD_EncodeSample + CFHD_DecodeSample loop over the frames -- the only way to do this before group batches existed,
  (b) cfhd_amd_batch_roundtrip passes of one batch of frames / 2 groups,
  (c) four such batches in flight on the frame queue (submit all, wait in order),
and the HIP-event time of every kernel slot of one pass of (b).  Warm-up passes first, then `passes` timed passes each; mean and spread (min .. max) in frames per second.
One process; the whole run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end.
  python tools/group_batch_throughput.py [frames=256] [passes=8] [limit=420]"""
import ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import group_batches as GB

W, H = 1920, 1080
GOP = T.ENCODING_FLAGS_2FRAME_GOP


def spread(fps):
    return {"mean": round(float(np.mean(fps)), 1), "min": round(float(min(fps)), 1), "max": round(float(max(fps)), 1), "passes": len(fps)}


def c_abi_loop(L, frames, pitch, n, passes, warmup=1):
    enc = ctypes.c_void_p(); dec = ctypes.c_void_p()
    assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0 and L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    assert L.CFHD_PrepareToEncode(enc, W, H, T.PIX_YUY2, T.ENCODED_YUV422, GOP, T.QUALITY_FILMSCAN1) == 0
    out = np.zeros(pitch * ((H + 7) // 8 * 8), np.uint8)
    prepared = False
    fps = []
    for k in range(warmup + passes):
        t0 = time.perf_counter()
        for i in range(n):
            f = frames[i % len(frames)]
            assert L.CFHD_EncodeSample(enc, f.ctypes.data_as(ctypes.c_void_p), pitch) == 0, T.amd_last_error()
            p = ctypes.c_void_p(); sz = ctypes.c_size_t()
            assert L.CFHD_GetSampleData(enc, ctypes.byref(p), ctypes.byref(sz)) == 0
            if not prepared:
                aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
                assert L.CFHD_PrepareToDecode(dec, 0, 0, T.PIX_YUY2, 1, 0, p, sz.value, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
                prepared = True
            assert L.CFHD_DecodeSample(dec, p, sz.value, out.ctypes.data_as(ctypes.c_void_p), pitch) == 0, T.amd_last_error()
        if k >= warmup: fps.append(n / (time.perf_counter() - t0))
    L.CFHD_CloseEncoder(enc); L.CFHD_CloseDecoder(dec)
    return fps


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 420
    signal.alarm(limit)                                   # the default action ends the process
    L = GB.lib()
    frames, pitch = T.qbist_frames(10, 32, W, H, T.PIX_YUY2) if T.have_ref() else ([T.synth_yuy2(W, H, 70 + i)[0] for i in range(32)], W * 2)
    result = {"frames_per_pass": n, "geometry": "%dx%d YUY2 FILMSCAN1 two-frame groups" % (W, H)}
    result["c_abi_loop_fps"] = spread(c_abi_loop(L, frames, pitch, n, max(2, passes // 2)))
    print("(a)", result["c_abi_loop_fps"], flush=True)

    def batch():
        b = L.cfhd_amd_batch_create_ex(W, H, T.PIX_YUY2, T.ENCODED_YUV422, GOP, T.QUALITY_FILMSCAN1, n, 1, 0)
        assert b, T.amd_last_error()
        for i in range(n): assert L.cfhd_amd_batch_upload(b, i, frames[i % len(frames)].ctypes.data_as(ctypes.c_void_p), pitch) == 0
        return b
    b = batch()
    fps = []
    for k in range(3 + passes):
        t0 = time.perf_counter()
        total = L.cfhd_amd_batch_roundtrip(b)
        assert total > 0, (total, T.amd_last_error())
        if k >= 3: fps.append(n / (time.perf_counter() - t0))
    result["batch_roundtrip_fps"] = spread(fps)
    result["sample_bytes_per_frame"] = int(total // n)
    slots = {0: "fwd level 1", 1: "fwd temporal + middle", 2: "fwd top", 5: "inv top", 4: "inv middle + temporal", 3: "inv last level", 8: "k_ent_count", 9: "k_ent_scan", 10: "k_ent_layout", 11: "k_ent_emit",
             12: "k_dec_parse_group", 13: "band decoder", 14: "k_dec_lowpass"}
    result["kernel_ms"] = {name: round(float(L.cfhd_amd_batch_kernel_ms(b, s)), 3) for s, name in slots.items()}
    result["kernel_names"] = [L.cfhd_amd_batch_kernel_name(b, s).decode() for s in range(6)]
    print("(b)", result["batch_roundtrip_fps"], result["kernel_ms"], flush=True)
    queue = [b] + [batch() for _ in range(3)]
    fps = []
    for k in range(2 + passes):
        t0 = time.perf_counter()
        for q in queue: assert L.cfhd_amd_batch_submit(q) == 0
        for q in queue: assert L.cfhd_amd_batch_wait(q) > 0, T.amd_last_error()
        if k >= 2: fps.append(len(queue) * n / (time.perf_counter() - t0))
    result["four_in_flight_fps"] = spread(fps)
    print("(c)", result["four_in_flight_fps"], flush=True)
    for q in queue: L.cfhd_amd_batch_destroy(q)
    signal.alarm(0)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
