#!/usr/bin/env python3
"""Throughput of the frame queue fed from device memory: 1920 x 1080 RG48 -> RGB 4:4:4 at FILMSCAN1, encode only, `frames` frames a pass (256: a batch's samples
share an arena of 4 GiB, which takes 343 frames of this size at the most), `depth` batches in flight (feed and submit all, wait in order), the frames in HBM -- the
RG48 pictures the decode queue makes of 32 distinct samples, so every leg encodes the same frames:
  (a) upload_device   `frames` calls of cfhd_amd_batch_upload_device a pass, from packed frames (runs on a library without the planar entry point too: the baseline),
  (b) planar_u16 / planar_f16 / planar_f32   ONE call of cfhd_amd_batch_upload_device_planar a pass, from a contiguous (n, 3, H, W) tensor of that element type,
  (c) chain           decode queue (samples in HBM, pictures delivered as PLANAR_F32 into device memory) -> cfhd_amd_batch_upload_device_planar -> frame queue, per
                      pass: nothing leaves HBM between the samples that go in and the samples that come out.
A run is sized by time: rounds of `depth` passes until `window` seconds have passed; every figure is frames per second over a run, mean and spread (min .. max) over
`repeats` runs, the legs run after run in turn.  Then, on ONE batch with nothing else in flight, the HIP-event times of k_enc_collect (cfhd_amd_batch_kernel_ms index
20) and, for the same layout, of k_dec_deliver (cfhd_amd_decode_batch_kernel_ms index 9), which moves the same bytes the other way: median (min .. max) over
`kernel_passes` passes, and the bytes read + written in that time.  CFHD_AMD_LIB names another build of the library: on one without the planar entry point only (a) runs.
The whole run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end, also written to `out` when given.
`emulated` as the last argument: a rehearsal on the CPU against the emulated library at 192 x 96 -- it checks the tool, its times mean nothing.
  python tools/planar_frames_throughput.py [frames=256] [depth=2] [window=3] [repeats=3] [limit=900] [out] [kernel_passes=9] [emulated]"""
import contextlib, ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import decode_queue as DQ
import group_batches as GB

V = ctypes.c_void_p
PACKED, U16, F16, F32 = 0, 1, 2, 3
NAMES = {U16: "planar_u16", F16: "planar_f16", F32: "planar_f32"}
ELEMENT = {U16: 2, F16: 2, F32: 4}


def spread(runs):
    fps = [f for f, _ in runs]
    return {"mean": round(float(np.mean(fps)), 1), "min": round(float(min(fps)), 1), "max": round(float(max(fps)), 1), "runs": len(fps), "window_seconds": [round(t, 2) for _, t in runs]}


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


class Hbm:
    """Device memory on the library's device (hipMalloc through the runtime the library loaded); under the emulator, host memory."""
    def __init__(self, emulated):
        self.hip = None if emulated else DQ.DeviceBlob(np.zeros(16, np.uint8)).hip
        self.held = []

    def alloc(self, nbytes):
        if self.hip is None:
            a = np.zeros(nbytes + 64, np.uint8); self.held.append(a)
            return a.ctypes.data + (-a.ctypes.data) % 64
        p = V(); assert self.hip.hipMalloc(ctypes.byref(p), nbytes) == 0, "hipMalloc of %d bytes" % nbytes
        self.held.append(p)
        return p.value

    def release(self):
        if self.hip is not None:
            for p in self.held: self.hip.hipFree(p)
        self.held = []


def main():
    args = sys.argv[1:]
    emulated = bool(args) and args[-1] == "emulated"
    if emulated: args = args[:-1]
    arg = lambda k, d: int(args[k]) if len(args) > k else d
    n, depth, window, repeats, limit, kernel_passes = arg(0, 256), arg(1, 2), arg(2, 3), arg(3, 3), arg(4, 900), arg(6, 9)
    out_path = args[5] if len(args) > 5 and args[5] != "-" else None
    W, H = (192, 96) if emulated else (1920, 1080)
    signal.alarm(limit)                                   # the default action ends the process
    with (T.emulated_product() if emulated else contextlib.nullcontext()):
        result = run(n, depth, window, repeats, kernel_passes, W, H, emulated)
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def run(n, depth, window, repeats, kernel_passes, W, H, emulated):
    L = DQ.lib(); GB.lib()
    planar = hasattr(L, "cfhd_amd_batch_upload_device_planar")
    L.cfhd_amd_batch_create_ex.restype = V
    L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32] + [ctypes.c_int] * 4
    L.cfhd_amd_batch_destroy.argtypes = [V]; L.cfhd_amd_batch_destroy.restype = None
    L.cfhd_amd_batch_upload_device.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
    L.cfhd_amd_batch_submit.argtypes = [V]
    L.cfhd_amd_batch_wait.restype = ctypes.c_longlong; L.cfhd_amd_batch_wait.argtypes = [V]
    L.cfhd_amd_batch_kernel_ms.restype = ctypes.c_float; L.cfhd_amd_batch_kernel_ms.argtypes = [V, ctypes.c_int]
    L.cfhd_amd_decode_batch_set_device_pictures.argtypes = [V, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    if planar: L.cfhd_amd_batch_upload_device_planar.argtypes = [V, ctypes.c_int, ctypes.c_int, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    hbm = Hbm(emulated)
    frames, pitch = T.qbist_frames(10, 32, W, H, T.PIX_YUY2) if T.have_ref() and not emulated else ([T.synth_yuy2(W, H, 70 + i)[0] for i in range(32)], W * 2)
    unique = T.amd_encode_frames(frames, pitch, W, H)
    samples = [unique[i % len(unique)] for i in range(n)]
    blob, offsets, sizes = DQ.pack(samples)
    owner, dblob = DQ.device_copy(blob)
    if dblob is None: dblob = owner.ptr
    c_off, c_size = DQ._sizes(offsets), DQ._sizes(sizes)
    frame_bytes = 6 * W * H
    result = {"geometry": "%dx%d RG48 -> RGB 4:4:4 FILMSCAN1, encode only; the frames: the decode queue's RG48 pictures of %d distinct 4:2:2 samples" % (W, H, len(unique)),
              "frames_per_pass": n, "passes_in_flight": depth, "window_seconds_asked": window, "planar_entry_point": planar, "emulated_rehearsal": emulated}

    # the decode queue: one batch per pass in flight (the chain's), each with device memory of its own -- large enough for the f32 tensor, which every layout reuses
    queues = [DQ.Queue(samples[0], "RG48", DQ.FULL, n) for _ in range(depth)]
    tensors = [hbm.alloc(n * 3 * H * W * 4) for _ in range(depth)]
    packed = hbm.alloc(n * frame_bytes)

    def deliver(k, target, layout):
        """One pass of decode queue k into `target` (None: nowhere), waited for."""
        q = queues[k]
        row = 6 * W if layout == PACKED else W * ELEMENT[layout]
        rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, target, (1 if layout == PACKED else 3) * H * row, row, layout)
        assert rc == 0, T.amd_last_error()
        assert L.cfhd_amd_decode_batch_submit_device(q.b, dblob, blob.nbytes, c_off, c_size, n) == 0, T.amd_last_error()
        assert L.cfhd_amd_decode_batch_wait(q.b, None) == n, T.amd_last_error()

    deliver(0, packed, PACKED)
    batches = []
    for _ in range(depth):
        b = L.cfhd_amd_batch_create_ex(W, H, T.PIX_RG48, T.ENCODED_RGB444, 0, T.QUALITY_FILMSCAN1, n, 1, 1)
        assert b, T.amd_last_error()
        batches.append(b)

    def timed(step, seconds):
        done = 0; t0 = time.perf_counter()
        while True:
            done += step()
            el = time.perf_counter() - t0
            if el >= seconds: return done / el, el

    sample_bytes = {}

    def feed(k, leg):
        b = batches[k]
        if leg == "upload_device":
            for i in range(n): assert L.cfhd_amd_batch_upload_device(b, i, packed + i * frame_bytes, 6 * W) == 0, T.amd_last_error()
        else:
            layout = F32 if leg == "chain" else leg
            row = W * ELEMENT[layout]
            assert L.cfhd_amd_batch_upload_device_planar(b, 0, n, tensors[k], 3 * H * row, row, layout) == 0, T.amd_last_error()

    def encode_run(leg, seconds, use=None):
        use = list(use) if use is not None else list(range(depth))
        def one_round():
            if leg == "chain":
                for k in use: deliver(k, tensors[k], F32)
            for k in use:
                feed(k, leg)
                assert L.cfhd_amd_batch_submit(batches[k]) == 0, T.amd_last_error()
            for k in use:
                total = L.cfhd_amd_batch_wait(batches[k])
                assert total > 0, (total, T.amd_last_error())
                sample_bytes.setdefault(leg, total)
                assert sample_bytes[leg] == total, "the passes of one leg encode the same frames"
            return len(use) * n
        return timed(one_round, seconds)

    def fill(layout):
        for k in range(depth): deliver(k, tensors[k], layout)
        for k in range(depth): assert L.cfhd_amd_decode_batch_set_device_pictures(queues[k].b, None, 0, 0, 0) == 0

    legs = ["upload_device"] + ([U16, F16, F32, "chain"] if planar else [])
    name = lambda leg: NAMES.get(leg, leg)
    fps = {name(leg): [] for leg in legs}
    for leg in legs:                                          # warm-up: every path once
        if leg in NAMES: fill(leg)
        encode_run(leg, 0)
    for r in range(repeats):                                  # run after run in turn: what drifts, drifts for all
        for leg in legs:
            if leg in NAMES: fill(leg)                         # (outside the timed window: the tensor is the caller's, made before)
            fps[name(leg)].append(encode_run(leg, window))
        print("repeat", r, {k: (round(x[-1][0], 1), round(x[-1][1], 2)) for k, x in fps.items()}, flush=True)
    result["fps"] = {k: spread(x) for k, x in fps.items()}
    result["sample_bytes_per_pass"] = {name(k): int(v) for k, v in sample_bytes.items()}
    if planar:
        # every way of feeding encodes the same frames: u16 and f32 give back the decode queue's words, so their samples have the size of the packed frames' samples
        assert sample_bytes[U16] == sample_bytes["upload_device"] == sample_bytes[F32] == sample_bytes["chain"], sample_bytes
        kernels = {"what": "one batch alone, nothing else in flight, HIP events, %d passes: median (min .. max) ms per %d frames; bytes = elements read + RG48 words written (k_enc_collect), "
                           "the other way round (k_dec_deliver)" % (kernel_passes, n)}
        for layout in (U16, F16, F32):
            moved = n * (3 * H * W * ELEMENT[layout] + frame_bytes)
            collect, deliver_ms = [], []
            for _ in range(kernel_passes):
                deliver(0, tensors[0], layout)
                deliver_ms.append(float(L.cfhd_amd_decode_batch_kernel_ms(queues[0].b, 9)))
                encode_run(layout, 0, use=[0])
                collect.append(float(L.cfhd_amd_batch_kernel_ms(batches[0], 20)))
            assert L.cfhd_amd_decode_batch_kernel_name(queues[0].b, 9) == b"k_dec_deliver"
            c, d = float(np.median(collect)), float(np.median(deliver_ms))
            kernels[NAMES[layout]] = {"bytes_moved_per_pass": int(moved), "k_enc_collect_ms": stats(collect), "k_enc_collect_tb_per_s": round(moved / (c * 1e-3) / 1e12, 3) if c > 0 else None,
                                      "k_dec_deliver_ms": stats(deliver_ms), "k_dec_deliver_tb_per_s": round(moved / (d * 1e-3) / 1e12, 3) if d > 0 else None,
                                      "collect_over_deliver": round(c / d, 3) if d > 0 else None}
        encode_run("upload_device", 0, use=[0])
        assert L.cfhd_amd_batch_kernel_ms(batches[0], 20) == 0, "a pass fed by upload_device has no collect time"
        result["kernels"] = kernels
    for b in batches: L.cfhd_amd_batch_destroy(b)
    for q in queues: q.close()
    hbm.release()
    del owner
    return result


if __name__ == "__main__":
    main()
