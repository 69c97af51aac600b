#!/usr/bin/env python3
"""Throughput of one GROUP encoder's stream on the frame queue (cfhd_amd_batch_create_group_stream): 1920 x 1080 YUY2, the benchmark's 32 Qbist frames in turn,
`frames` frames a pass (frames 2 g and 2 g + 1 form group g), at HIGH and at FILMSCAN2 -- words whose group tables follow the key samples --, mode 1 (encode only)
and mode 0 (round trip), the frames resident in HBM, warmed up; a run is sized by TIME as in tools/stream_batches_throughput.py, `repeats` runs of each variant, one
variant after the other, all in one process:
  (a) one_handle      one CFHD_EncodeSample handle prepared with the group flag over the same frames from plain memory (encode only), and the same loop with one
                      CFHD_DecodeSample handle behind it (round trip) -- the only way to a group stream at these words before,
  (b) one_stream      one group-stream batch, one pass at a time (submit, wait),
  (c) four_streams    `depth` group-stream batches in flight (submit all, wait in order): independent streams.
For every pass of (b) and (c) cfhd_amd_batch_stream_stats is recorded (rounds, frames coded); the figures of a variant are frames of the STREAM per second, the
frames coded again are its cost, not its yield.  Beside them:
  static_word     FILMSCAN1 round trips through cfhd_amd_batch_create_group_stream against cfhd_amd_batch_create_groups, `depth` in flight, fresh batches for every
                  run, the two entries in alternating runs;
  worst_material  a stream that alternates 16 Qbist frames with 16 frames of noise (+-5) on them and never repeats a pass: rounds and frames coded a pass.
The whole run ends itself after `limit` seconds (SIGALRM) rather than hang.  One JSON line at the end, also written to `out` when given.
  python tools/group_stream_throughput.py [frames=256] [depth=4] [window=3] [repeats=3] [limit=900] [out] [sections=words,static,worst]"""
import ctypes, json, os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cfhd_testlib as T
import group_stream_batches as G
from group_batches_rgb8_throughput import spread, timed
from stream_batches_throughput import passes

W, H = 1920, 1080
V = ctypes.c_void_p
DISTINCT = 32
WORDS = {"HIGH": G.HIGH, "FILMSCAN2": G.FILMSCAN2}


def noisy(frames):
    """The worst material tried: runs of 16 frames as they are and 16 with uniform noise of +-5 on them, in turn.  (With the +-10 of tools/stream_batches_throughput.py
    the first pass at FILMSCAN2 fails with -9: a group of two such frames reaches 80 % of the sample buffer, where the reference codes bands as zeros.)"""
    rng = np.random.default_rng(11)
    out = []
    for i, f in enumerate(frames):
        if (i // 16) % 2 == 0: out.append(f); continue
        out.append(np.clip(f.astype(np.int16) + rng.integers(-5, 6, f.shape), 0, 255).astype(np.uint8))
    return out


def make(L, entry, quality, n, mode, frames, pitch):
    create = L.cfhd_amd_batch_create_group_stream if entry == "group_stream" else L.cfhd_amd_batch_create_groups
    b = create(W, H, T.PIX_YUY2, 0, quality, n, 1, mode)
    assert b, T.amd_last_error()
    for i in range(n): assert L.cfhd_amd_batch_upload(b, i, np.asarray(frames[i % len(frames)]).ctypes.data_as(V), pitch) == 0
    return b


def run_batches(L, bs, n, window, repeats, stats):
    """`repeats` runs over the batches in flight together; stats: a list that takes [rounds, frames coded, groups with other tables] of every pass (None: a create_groups batch)."""
    def one_round():
        for b in bs: assert L.cfhd_amd_batch_submit(b) == 0, T.amd_last_error()
        for b in bs:
            total = L.cfhd_amd_batch_wait(b)
            assert total > 0, (total, T.amd_last_error())
            if stats is not None:
                out = (ctypes.c_int * 3)()
                assert L.cfhd_amd_batch_stream_stats(b, out) == 0
                stats.append(list(out))
        return len(bs) * n
    before = len(stats) if stats is not None else 0
    one_round(); one_round()                              # warm-up: every batch twice (the second pass of a stream guesses from the first)
    warm = len(stats) - before if stats is not None else 0
    return [timed(one_round, window) for _ in range(repeats)], warm


def measure_handle(L, name, window, repeats, frames, pitch):
    """(a): one encoder handle with the group flag, and the same with one decoder handle behind it (every sample decoded: group -> frame 0, P-frame sample -> frame 1)."""
    out = {}
    for decode in (False, True):
        enc = V(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
        assert L.CFHD_PrepareToEncode(enc, W, H, T.PIX_YUY2, T.ENCODED_YUV422, G.GOP, WORDS[name]) == 0
        ptrs = [np.asarray(f).ctypes.data_as(V) for f in frames]
        dec = V(); prepared = [False]; picture = np.zeros(pitch * H, np.uint8)
        if decode: assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
        def calls():
            for p in ptrs:
                assert L.CFHD_EncodeSample(enc, p, pitch) == 0, T.amd_last_error()
                if not decode: continue
                d = V(); sz = ctypes.c_size_t()
                assert L.CFHD_GetSampleData(enc, ctypes.byref(d), ctypes.byref(sz)) == 0
                if sz.value == 40: continue                 # (the sequence header)
                if not prepared[0]:
                    aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
                    assert L.CFHD_PrepareToDecode(dec, 0, 0, T.PIX_YUY2, 1, 0, d, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
                    prepared[0] = True
                assert L.CFHD_DecodeSample(dec, d, sz.value, picture.ctypes.data_as(V), pitch) == 0, T.amd_last_error()
            return len(ptrs)
        calls()
        out["round_trip" if decode else "encode_only"] = {"fps": spread([timed(calls, window) for _ in range(repeats)])}
        L.CFHD_CloseEncoder(enc)
        if decode: L.CFHD_CloseDecoder(dec)
    print(name, "one_handle", out, flush=True)
    return out


def measure_word(L, name, n, depth, window, repeats, frames, pitch):
    out = {"one_handle": measure_handle(L, name, window, repeats, frames, pitch)}
    for mode in (1, 0):
        res = {}
        for variant, k in (("one_stream", 1), ("four_streams", depth)):
            bs = [make(L, "group_stream", WORDS[name], n, mode, frames, pitch) for _ in range(k)]
            stats = []
            runs, warm = run_batches(L, bs, n, window, repeats, stats)
            res[variant] = {"fps": spread(runs), "batches_in_flight": k, "warm_up_passes": passes(stats[:warm], n), "timed_passes": passes(stats[warm:], n)}
            print(name, "mode", mode, variant, res[variant], flush=True)
            for b in bs: L.cfhd_amd_batch_destroy(b)
        out["mode_%d" % mode] = res
    return out


def measure_static(L, n, depth, window, repeats, frames, pitch):
    """FILMSCAN1 through either entry, mode 0, `depth` batches in flight; only one entry's batches are alive at a time, made afresh for every run, and the entry that goes
    first alternates (tools/stream_batches_throughput.py measure_static says why)."""
    runs = {"groups": [], "group_stream": []}
    for r in range(repeats):
        for e in (("groups", "group_stream") if r % 2 == 0 else ("group_stream", "groups")):
            bs = [make(L, e, T.QUALITY_FILMSCAN1, n, 0, frames, pitch) for _ in range(depth)]
            got, _ = run_batches(L, bs, n, window, 1, [] if e == "group_stream" else None)
            runs[e] += got
            for b in bs: L.cfhd_amd_batch_destroy(b)
    return {"what": "FILMSCAN1, mode 0, %d batches in flight, alternating runs, fresh batches for every run" % depth, "create_groups": spread(runs["groups"]), "create_group_stream": spread(runs["group_stream"])}


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    n, depth, window, repeats, limit = arg(1, 256), arg(2, 4), arg(3, 3), arg(4, 3), arg(5, 900)
    out_path = sys.argv[6] if len(sys.argv) > 6 and sys.argv[6] != "-" else None
    signal.alarm(limit)                                   # the default action ends the process
    L = G.lib()
    frames, pitch = T.qbist_frames(10, DISTINCT, W, H, T.PIX_YUY2)
    result = {"geometry": "%dx%d YUY2 two-frame groups, %d Qbist frames (seed 10) in turn, frames of the stream per second" % (W, H, DISTINCT), "frames_per_pass": n, "window_seconds_asked": window}
    sections = sys.argv[7].split(",") if len(sys.argv) > 7 else ["words", "static", "worst"]
    for name in WORDS if "words" in sections else (): result[name] = measure_word(L, name, n, depth, window, repeats, frames, pitch)
    if "static" in sections:
        result["static_word"] = measure_static(L, n, depth, window, repeats, frames, pitch)
        print("static word", result["static_word"], flush=True)
    # a stream that never repeats: every pass takes the material a few groups further on (fed again before the pass, outside any timing), so that the guess a pass
    # starts from -- the tables of the pass before, group by group -- meets the runs of noise in other places
    worst = {}
    material = noisy(frames)
    for name in WORDS if "worst" in sections else ():
        b = make(L, "group_stream", WORDS[name], n, 1, material, pitch)
        stats = []
        for k in range(4):
            for i in range(n): assert L.cfhd_amd_batch_upload(b, i, np.asarray(material[(i + 6 * k) % len(material)]).ctypes.data_as(V), pitch) == 0
            total = L.cfhd_amd_batch_roundtrip(b)
            assert total > 0, (name, k, total, T.amd_last_error())
            out = (ctypes.c_int * 3)(); assert L.cfhd_amd_batch_stream_stats(b, out) == 0
            stats.append(list(out))
        worst[name] = {"per_pass": stats, **passes(stats, n)}
        L.cfhd_amd_batch_destroy(b)
        print(name, "worst material", worst[name], flush=True)
    if "worst" in sections: result["worst_material"] = {"what": "16 Qbist frames, 16 with uniform noise of +-5 on them, in turn, moved on by 6 frames from pass to pass; one group-stream batch, mode 1; [rounds, frames coded, groups with other tables] of every pass", **worst}
    signal.alarm(0)
    if out_path:
        with open(out_path, "w") as fh: fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
