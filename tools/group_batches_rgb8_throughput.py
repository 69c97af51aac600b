#!/usr/bin/env python3
"""Throughput of the frame queue over two-frame groups from 8-bit RGB (cfhd_amd_batch_create_groups): 1920 x 1080, 32 distinct frames of RG24 and of BGRA at
FILMSCAN1, `groups` groups a pass (2 * groups frames, the 32 in turn), `depth` batches in flight (submit all, wait in order), warmed up; a run is sized by TIME as in
tools/decode_queue_groups_throughput.py, `repeats` runs of each variant, one variant after the other, all in one process:
  (a) encode_resident   mode 1, the frames already in HBM (cfhd_amd_batch_submit),
  (b) encode_host_fed   mode 1, the frames in one registered host blob (cfhd_amd_batch_submit_host), the samples to the host,
  (c) roundtrip         mode 0, the frames in HBM, the pictures left in HBM.
Beside them, in the same call: (d) one CFHD_EncodeSample handle over the same frames -- this build of the library and, when `parent_lib` names one, the build of the
parent commit (each in a child process of its own, CFHD_AMD_LIB, the two in turn) --, and (a) and (c) for YUY2-source groups (subband 7 as raw words: no two-pass
coding).  Every figure is frames per second over a run; mean and spread (min .. max) over the runs.  Also the HIP-event time of the entropy coder's slots
(cfhd_amd_batch_kernel_ms 8 .. 11; 8 holds k_ent_split_two_pass + k_ent_count) and, for (c), of the band decoder (13, with k_dec_band_two_pass) over `kernel_passes`
passes on ONE batch with nothing else in flight.  The whole run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end, also written
to `out` when given.
  python tools/group_batches_rgb8_throughput.py [groups=256] [depth=4] [window=3] [repeats=3] [limit=900] [out] [kernel_passes=5] [parent_lib]"""
import ctypes, json, os, signal, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import group_batches as GB
import gop_input_frames

W, H = 1920, 1080
V = ctypes.c_void_p
DISTINCT = 32


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


def source_frames(name):
    """32 frames of a moving picture: one frame of the group encoder's test pictures (tests/gop_input_frames.py; YUY2: synth_yuy2), panned by (4, 2) pixels a frame."""
    base, pitch = T.synth_yuy2(W, H, 70) if name == "YUY2" else gop_input_frames.frame(name, W, H, 5)
    img = np.asarray(base).reshape(H, pitch)
    px = 4 if name == "YUY2" else pitch // W          # (YUY2: two pixels in four bytes -- pan by whole pairs)
    return [np.ascontiguousarray(np.roll(np.roll(img, 2 * i, axis=0), 4 * px * i // (2 if name == "YUY2" else 1), axis=1)).reshape(-1) for i in range(DISTINCT)], pitch


def lib():
    L = GB.lib()
    L.cfhd_amd_batch_create_groups.restype = V
    L.cfhd_amd_batch_create_groups.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_int] * 4
    L.cfhd_amd_register_host_buffer.argtypes = [V, ctypes.c_size_t]; L.cfhd_amd_unregister_host_buffer.argtypes = [V]
    return L


def measure_queue(L, name, ng, depth, window, repeats, kernel_passes, variants):
    frames, pitch = source_frames(name)
    n = 2 * ng
    fbytes = pitch * H
    out = {"source": "%dx%d %s FILMSCAN1, %d distinct frames" % (W, H, name, DISTINCT)}
    def batches(mode, resident):
        bs = []
        for _ in range(depth):
            b = L.cfhd_amd_batch_create_groups(W, H, GB.FOURCCS[name], 0, T.QUALITY_FILMSCAN1, n, 1, mode)
            assert b, T.amd_last_error()
            if resident:
                for i in range(n): assert L.cfhd_amd_batch_upload(b, i, np.asarray(frames[i % DISTINCT]).ctypes.data_as(V), pitch) == 0
            bs.append(b)
        return bs
    # one variant after the other: its `depth` batches live only while it is measured (a batch of 256 groups holds its frames, two pyramids and its samples in HBM and
    # as much pinned host memory again)
    blob = None
    out["fps"] = {}; out["kernel_ms"] = {}
    slots = {8: "k_ent_split_two_pass + k_ent_count" if name != "YUY2" else "k_ent_count", 9: "k_ent_scan", 10: "k_ent_sizes + k_ent_pack_offsets + k_ent_layout", 11: "k_ent_emit"}
    for v in variants:
        mode, resident = (0, True) if v == "roundtrip" else (1, v == "encode_resident")
        bs = batches(mode, resident)
        if not resident and blob is None:
            blob = np.zeros(n * fbytes, np.uint8)
            for i in range(n): blob[i * fbytes: (i + 1) * fbytes] = np.asarray(frames[i % DISTINCT])
            assert L.cfhd_amd_register_host_buffer(blob.ctypes.data_as(V), blob.nbytes) == 0
        def run(seconds, use):
            def one_round():
                for b in use:
                    rc = L.cfhd_amd_batch_submit(b) if v != "encode_host_fed" else L.cfhd_amd_batch_submit_host(b, blob.ctypes.data_as(V), fbytes, pitch, None, 0, 0)
                    assert rc == 0, (rc, T.amd_last_error())
                for b in use:
                    total = L.cfhd_amd_batch_wait(b)
                    assert total > 0, (total, T.amd_last_error())
                return len(use) * n
            return timed(one_round, seconds)
        run(0, bs)                                            # warm-up: every batch once
        runs = [run(window, bs) for _ in range(repeats)]
        out["fps"][v] = spread(runs)
        print(name, v, out["fps"][v], flush=True)
        if v != "encode_host_fed":
            # the kernel slots: passes on one batch alone, nothing else in flight on the device
            ks = dict(slots)
            if v == "roundtrip": ks[13] = "band decoder" + (" (with k_dec_band_two_pass)" if name != "YUY2" else "")
            per = []
            for _ in range(kernel_passes):
                run(0, bs[:1])
                per.append([float(L.cfhd_amd_batch_kernel_ms(bs[0], k)) for k in ks])
            per = np.array(per)
            out["kernel_ms"][v] = {"what": "one batch of %d groups alone, %d passes: median (min .. max)" % (ng, kernel_passes),
                                   **{"%d %s" % (k, t): {"median": round(float(np.median(per[:, i])), 4), "min": round(float(per[:, i].min()), 4), "max": round(float(per[:, i].max()), 4)} for i, (k, t) in enumerate(ks.items())}}
        if "first_group_sample_bytes" not in out:
            p = V(); sz = ctypes.c_size_t()
            assert L.cfhd_amd_batch_get_sample(bs[0], 0, ctypes.byref(p), ctypes.byref(sz)) == 0
            out["first_group_sample_bytes"] = int(sz.value)
        for b in bs: L.cfhd_amd_batch_destroy(b)
    if blob is not None: L.cfhd_amd_unregister_host_buffer(blob.ctypes.data_as(V))
    return out


def handle_child(window):
    """One CFHD_EncodeSample handle per input over the 32 frames in turn, whatever library CFHD_AMD_LIB names: frames per second over one window each."""
    out = {}
    L = T.product()
    for name in ("RG24", "BGRA"):
        frames, pitch = source_frames(name)
        enc = V(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
        assert L.CFHD_PrepareToEncode(enc, W, H, GB.FOURCCS[name], T.ENCODED_YUV422, GB.GOP, T.QUALITY_FILMSCAN1) == 0
        ptrs = [np.asarray(f).ctypes.data_as(V) for f in frames]
        def calls():
            for p in ptrs: assert L.CFHD_EncodeSample(enc, p, pitch) == 0, T.amd_last_error()
            return len(ptrs)
        calls()
        fps, el = timed(calls, window)
        out[name] = [round(fps, 1), round(el, 2)]
        L.CFHD_CloseEncoder(enc)
    print("HANDLE " + json.dumps(out))


def measure_handles(parent_lib, window, repeats):
    builds = [("this_commit", None)] + ([("parent_commit", parent_lib)] if parent_lib else [])
    runs = {b: {"RG24": [], "BGRA": []} for b, _ in builds}
    for r in range(repeats):
        for b, path in builds:
            env = dict(os.environ)
            if path: env["CFHD_AMD_LIB"] = path
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--handle", str(window)], env=env, capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
            got = json.loads(next(line for line in res.stdout.splitlines() if line.startswith("HANDLE "))[7:])
            for name in got: runs[b][name].append(tuple(got[name]))
            print("handle", b, "repeat", r, got, flush=True)
    return {b: {name: spread(x) for name, x in per.items()} for b, per in runs.items()}


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--handle": return handle_child(float(sys.argv[2]))
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    ng, depth, window, repeats, limit = arg(1, 256), arg(2, 4), arg(3, 3), arg(4, 3), arg(5, 900)
    out_path = sys.argv[6] if len(sys.argv) > 6 and sys.argv[6] != "-" else None
    kernel_passes = arg(7, 5)
    parent_lib = sys.argv[8] if len(sys.argv) > 8 else None
    signal.alarm(limit)                                   # the default action ends the process
    L = lib()
    result = {"geometry": "%dx%d two-frame groups at FILMSCAN1, frames per second" % (W, H), "groups_per_pass": ng, "frames_per_pass": 2 * ng, "passes_in_flight": depth, "window_seconds_asked": window}
    for name in ("RG24", "BGRA"):
        result[name.lower() + "_source"] = measure_queue(L, name, ng, depth, window, repeats, kernel_passes, ("encode_resident", "encode_host_fed", "roundtrip"))
    result["yuy2_source"] = measure_queue(L, "YUY2", ng, depth, window, repeats, kernel_passes, ("encode_resident", "roundtrip"))
    result["one_handle"] = {"what": "one CFHD_EncodeSample handle over the same %d frames in turn, plain host memory, a child process per build and repeat" % DISTINCT,
                            **measure_handles(parent_lib, window, repeats)}
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
