"""One encoder's stream on the frame queue, rate feedback included -- cfhd_amd_batch_create_stream / cfhd_amd_batch_stream_stats: the helpers and test bodies shared by
tests/test_gpu_stream_batches.py (hardware) and tests/test_stream_batches_emulated.py (the same functions inside cfhd_testlib.emulated_product()).

What is checked against what:
  samples   the batch's samples, pass behind pass, against ONE CFHD_EncodeSample handle of this library fed the same frames (amd_encode_frames) and against the
            reference encoder driven the same way (ref_encode_frames): equal sizes, equal bytes after mask_volatile_metadata (quality_matrix.assert_samples_equal).
  tables    every sample's divisors (hooks: cfhd_amd_sample_quants) against the host derivation walked over the sizes (cfhd_amd_quant_sequence).
  stats     cfhd_amd_batch_stream_stats against the table changes counted in the reference's own stream.
  pictures  (mode 0) one CFHD_DecodeSample handle over the same samples (decode_queue.handle_pictures): 16-bit outputs byte for byte, 8-bit 4:2:2 within the one dither step.
The inputs are judged on the reference's samples alone, on the CPU, before the product is asked anything (check_input_does_its_job, limiter_input_does_its_job).
Test infrastructure only: nothing here is a product path."""
import ctypes, os, subprocess, sys
import numpy as np
from cfhd_testlib import *
import quality_matrix as Q
import group_batches as GB
import decode_queue as DQ

V = ctypes.c_void_p
FILMSCAN2, FILMSCAN3, MEDIUM, HIGH = 5, 6, 2, 3
INTERLACED, GOP = 1, ENCODING_FLAGS_2FRAME_GOP
W, H, N, PASSES = 192, 96, 8, 3
# route: (input, encoded format, encoding flags, strip kernels forced) -- quality_matrix.ROUTES' triples; YUY2 once more with the strip kernels, and interlaced
ROUTES = {"YUY2-422": ("YUY2", "422", 0, False), "YUY2-422-strips": ("YUY2", "422", 0, True), "YUY2-422i": ("YUY2", "422", INTERLACED, False),
          "RG48-444": ("RG48", "444", 0, False), "b64a-4444": ("b64a", "4444", 0, False), "BYR4-bayer": ("BYR4", "bayer", 0, False)}
STREAM_CASES = [(r, q) for r in ROUTES for q in (FILMSCAN2, FILMSCAN3)]
BYTES = {"YUY2": 2, "RG48": 6, "b64a": 8, "BYR4": 2}
# The noise amplitude (in 8-bit steps, uniform in [-a, a]) of the frame at stream index i of pass k is SCHEDULE[(i + ROTATION k) % 8]: flat runs with noisy frames
# between them, rotated by two frames from pass to pass.  The FILMSCAN2 / 3 limiter (cfhd_tables.cpp derive_subband_tables) steps down behind a flat frame --
# compression beyond 5.5 / 4.5 -- by up to 4 steps and up behind a noisy one -- below 4 / 3 -- by up to 7, inside 0 .. 20: a long run of one kind saturates it and the
# tables stand still, a change of kind moves them again; stronger noise (48) saturates it within two frames on every route.  Found by trying schedules against the
# reference encoder alone until check_input_does_its_job held on every route at both words.
SCHEDULE, ROTATION = (0, 16, 0, 0, 0, 0, 0, 6), 2


def lib():
    L = GB.lib()
    if not getattr(L, "_stream_batches_declared", False):
        L.cfhd_amd_batch_create_stream.restype = V
        L.cfhd_amd_batch_create_stream.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32] + [ctypes.c_int] * 4
        L.cfhd_amd_batch_stream_stats.argtypes = [V, ctypes.POINTER(ctypes.c_int)]
        L.cfhd_amd_quantizer_is_static.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
        L.cfhd_amd_register_host_buffer.argtypes = [V, ctypes.c_size_t]; L.cfhd_amd_unregister_host_buffer.argtypes = [V]
        L._stream_batches_declared = True
    return L


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def noisy_frame(fmt, w, h, index, amplitude, interlaced=False):
    """Gradients plus uniform noise of the given amplitude (8-bit steps), as the input's bytes.  The gradients move a little with the index, so that no two frames of a
    stream are equal; interlaced: the second field a few pixels later."""
    rng = np.random.default_rng(900 + index)
    y, x = np.mgrid[0:h, 0:w]
    planes = {"YUY2": 3, "RG48": 3, "b64a": 4, "BYR4": 1}[fmt]
    comps = []
    for k in range(planes):
        g = 128.0 + (36.0 - 6.0 * k) * np.sin((x + 3.0 * index) / (61.0 + 17.0 * k)) * np.cos((y + 5.0 * k) / (47.0 + 11.0 * k))
        if interlaced: g[1::2] = np.roll(g[1::2], 2, axis=1)
        comps.append(g + (rng.integers(-amplitude, amplitude + 1, (h, w)) if amplitude else 0))
    if fmt == "YUY2":
        f = np.zeros((h, w * 2), np.uint8)
        f[:, 0::2] = np.clip(comps[0], 0, 255); f[:, 1::4] = np.clip(comps[1][:, 0::2], 0, 255); f[:, 3::4] = np.clip(comps[2][:, 0::2], 0, 255)
    elif fmt == "BYR4":
        gain = np.where((y % 2 == 0) & (x % 2 == 0), 0.8, np.where((y % 2 == 1) & (x % 2 == 1), 0.6, 1.0))      # (red-green order: R and B darker than the greens)
        f = np.clip(comps[0] * gain * 200.0, 0, 65535).astype(np.uint16).view(np.uint8)
    else:
        f = np.stack([np.clip(c * 256.0, 0, 65535).astype(np.uint16) for c in comps], axis=2).reshape(h, -1).view(np.uint8)
    f = np.ascontiguousarray(f).reshape(-1)
    f.setflags(write=False)
    return f


def amplitude(index, nframes=N): return SCHEDULE[(index % nframes + ROTATION * (index // nframes)) % len(SCHEDULE)]


_streams = {}


def stream(route, quality):
    """(frames of PASSES passes, pitch, the reference's samples of the whole stream through one handle) -- computed once, shared, read-only."""
    key = (route, quality)
    if key not in _streams:
        fmt, enc, flags, _ = ROUTES[route]
        frames = [noisy_frame(fmt, W, H, i, amplitude(i), bool(flags & INTERLACED)) for i in range(N * PASSES)]
        pitch = W * BYTES[fmt]
        refs = ref_encode_frames(frames, pitch, W, H, pixfmt=fourcc(fmt), encoded=Q.ENCODED[enc], quality=quality, flags=flags)
        check_input_does_its_job(refs, N, "%s 0x%x" % (route, quality))
        _streams[key] = (frames, pitch, refs)
    return _streams[key]


def sample_tables(sample):
    out = (ctypes.c_int * 64)()
    a = np.frombuffer(sample, np.uint8).copy()
    n = hooks().cfhd_amd_sample_quants(p8(a), len(sample), out)
    assert n > 0, "cfhd_amd_sample_quants -> %d" % n
    return tuple(out[:n])


def table_changes(samples):
    """[i for which sample i carries other tables than sample i - 1], over a whole stream."""
    t = [sample_tables(s) for s in samples]
    return [i for i in range(1, len(t)) if t[i] != t[i - 1]]


def check_input_does_its_job(refs, nframes, what):
    """On the REFERENCE's samples alone: at least three distinct table sets, a change in each direction, and a change across every pass boundary."""
    t = [sample_tables(s) for s in refs]
    assert len(set(t)) >= 3, "%s: %d distinct table sets in the stream" % (what, len(set(t)))
    ups = [i for i in range(1, len(t)) if sum(t[i]) > sum(t[i - 1])]; downs = [i for i in range(1, len(t)) if sum(t[i]) < sum(t[i - 1])]
    assert ups and downs, "%s: tables coarser behind %s, finer behind %s" % (what, ups, downs)
    for k in range(nframes, len(t), nframes): assert t[k] != t[k - 1], "%s: the tables stand still across the boundary in front of frame %d" % (what, k)


# ------------------------------------------------------------------------------------------
# the batch
# ------------------------------------------------------------------------------------------
class Batch(GB.Batch):
    """One stream batch (or, entry="ex", one batch of cfhd_amd_batch_create_ex with the same arguments) with nframes slots; feed() puts a pass's frames into HBM."""
    def __init__(self, w, h, fmt, enc, flags, quality, nframes, mode, entry="stream"):
        self.L = lib(); self.w, self.h, self.name, self.n, self.mode = w, h, fmt, nframes, mode
        create = self.L.cfhd_amd_batch_create_stream if entry == "stream" else self.L.cfhd_amd_batch_create_ex
        self.b = create(w, h, fourcc(fmt), Q.ENCODED[enc], flags, quality, nframes, 1, mode)
        assert self.b, "cfhd_amd_batch_create_%s -> NULL (%s)" % (entry, amd_last_error())
        self.pitch = w * BYTES[fmt]

    def feed(self, frames):
        assert len(frames) == self.n
        for i, f in enumerate(frames):
            assert self.L.cfhd_amd_batch_upload(self.b, i, np.asarray(f).ctypes.data_as(V), self.pitch) == 0, amd_last_error()

    def stats(self):
        out = (ctypes.c_int * 3)(-7, -7, -7)
        rc = self.L.cfhd_amd_batch_stream_stats(self.b, out)
        return rc, list(out)

    def pictures(self):
        out = []
        for i in range(self.n):
            o = np.full(self.pitch * self.h, 7, np.uint8)
            assert self.L.cfhd_amd_batch_download_output(self.b, i, o.ctypes.data_as(V), self.pitch) == 0, amd_last_error()
            out.append(o)
        return out


def run_stream(bt, frames, passes, queued=False):
    """[(samples, stats, pictures or None)] of `passes` passes over consecutive runs of bt.n frames."""
    out = []
    for k in range(passes):
        bt.feed(frames[k * bt.n: (k + 1) * bt.n])
        if queued:
            assert bt.L.cfhd_amd_batch_submit(bt.b) == 0, amd_last_error()
            total = bt.L.cfhd_amd_batch_wait(bt.b)
        else: total = bt.L.cfhd_amd_batch_roundtrip(bt.b)
        assert total > 0, "pass %d -> %d (%s)" % (k, total, amd_last_error())
        s = bt.samples()
        assert total == sum(len(x) for x in s)
        rc, st = bt.stats()
        assert rc == 0, "cfhd_amd_batch_stream_stats -> %d" % rc
        out.append((s, st, bt.pictures() if bt.mode == 0 else None))
    return out


def check_pictures(samples, pictures, fmt, what):
    """The batch's pictures against one CFHD_DecodeSample handle over the same samples: 16-bit outputs byte for byte, 8-bit 4:2:2 within the one dither step."""
    want, geometry = DQ.handle_pictures(samples, fmt, DQ.FULL)
    for i, (rc, pic) in enumerate(want):
        assert rc == 0 and pic.size == pictures[i].size, (what, i, rc, geometry)
        if fmt == "YUY2":
            d = np.abs(pictures[i].astype(np.int16) - pic.astype(np.int16))
            assert d.max() <= 1, "%s picture %d: %d bytes further than one dither step from the handle's" % (what, i, int((d > 1).sum()))
        else: assert np.array_equal(pictures[i], pic), "%s picture %d: %d bytes differ from the handle's picture" % (what, i, int((pictures[i] != pic).sum()))


# ------------------------------------------------------------------------------------------
# 1. FILMSCAN2 / FILMSCAN3 streams
# ------------------------------------------------------------------------------------------
def check_stream(route, quality):
    fmt, enc, flags, strips = ROUTES[route]
    what = "%s 0x%x: " % (route, quality)
    frames, pitch, refs = stream(route, quality)
    mode = 1 if enc == "bayer" else 0
    L = lib()
    assert L.cfhd_amd_quantizer_is_static(W, H, fourcc(fmt), Q.ENCODED[enc], flags, quality) == 0
    class nothing:
        def __enter__(self): pass
        def __exit__(self, *a): pass
    with (Q.strip_shapes() if strips else nothing()):
        bt = Batch(W, H, fmt, enc, flags, quality, N, mode)
        try:
            assert bt.stats()[0] == -1                  # (no pass has completed)
            passes = run_stream(bt, frames, PASSES, queued=True)
        finally:
            bt.close()
        handle = amd_encode_frames(frames, pitch, W, H, fourcc(fmt), encoded=Q.ENCODED[enc], quality=quality, flags=flags)
    mine = [s for p in passes for s in p[0]]
    assert len(mine) == N * PASSES
    Q.assert_samples_equal(mine, handle, what + "against this library's handle: ")
    Q.assert_samples_equal(mine, refs, what + "against the reference: ")
    # every sample carries the tables the host derivation gives its place in the stream
    sizes = (ctypes.c_longlong * len(mine))(*[len(s) for s in mine])
    nq = len(sample_tables(mine[0]))
    seq = (ctypes.c_int * (nq * len(mine)))()
    plan_kind = PIXKIND[fmt]; plan_enc = ENC[enc]
    assert hooks().cfhd_amd_quant_sequence(W, H, plan_kind, plan_enc, quality, 0 if flags & INTERLACED else 1, sizes, len(mine), seq) == nq * len(mine)
    for f, s in enumerate(mine): assert sample_tables(s) == tuple(seq[nq * f: nq * f + nq]), what + "frame %d carries other tables than the derivation" % f
    stats = [p[1] for p in passes]
    assert sum(st[2] for st in stats) == len(table_changes(refs)), what + "stats %s, table changes in the reference's stream behind %s" % (stats, table_changes(refs))
    assert any(st[0] >= 2 for st in stats), what + "no pass took a second round: %s" % stats
    for st in stats: assert N <= st[1] <= N * st[0], what + "stats %s" % stats
    if mode == 0:
        for k, p in enumerate(passes): check_pictures(p[0], p[2], fmt, what + "pass %d" % k)


# ------------------------------------------------------------------------------------------
# 2. a pass that stands still; 3. static words through the new entry (the traces: tests/test_stream_batches_emulated.py)
# ------------------------------------------------------------------------------------------
def settle(bt, frame, limit=6):
    """Passes over nframes copies of one frame until the tables stop moving -- the FILMSCAN2 / 3 limiter moves at least a step a frame while the sample size lies outside
    its band and spans 0 .. 20, so 6 passes of 8 frames are enough --; returns the stats of every pass."""
    stats = []
    for k in range(limit):
        bt.feed([frame] * bt.n)
        assert bt.L.cfhd_amd_batch_roundtrip(bt.b) > 0, amd_last_error()
        rc, st = bt.stats()
        assert rc == 0
        stats.append(st)
        if st[2] == 0 and k: return stats
    raise AssertionError("the tables still move after %d passes over one frame: %s" % (limit, stats))


def check_still_pass():
    frame = noisy_frame("YUY2", W, H, 0, 6)
    bt = Batch(W, H, "YUY2", "422", 0, FILMSCAN2, N, 1)
    try:
        stats = settle(bt, frame)
        for k in range(2):
            bt.feed([frame] * N)
            assert bt.L.cfhd_amd_batch_roundtrip(bt.b) > 0, amd_last_error()
            assert bt.stats() == (0, [1, N, 0]), (stats, bt.stats())
        tail = bt.samples()
    finally:
        bt.close()
    # (and the settled stream is still the handle's: its last pass against the end of one handle's stream of as many copies)
    handle = amd_encode_frames([frame] * (N * (len(stats) + 2)), W * 2, W, H, quality=FILMSCAN2)
    Q.assert_samples_equal(tail, handle[-N:], "the settled pass against the handle: ")


STATIC_CASES = ["YUY2-422", "RG48-444"]


def check_static_word(route):
    """FILMSCAN1 through the new entry: cfhd_amd_batch_create_ex's samples (GUID pinned, DATE / TIME masked), stats [1, n, 0]."""
    fmt, enc, flags, _ = ROUTES[route]
    L = lib()
    L.cfhd_amd_set_clip_guid(bytes(range(16)))
    frames = [noisy_frame(fmt, W, H, i, 6) for i in range(2 * N)]
    mine = Batch(W, H, fmt, enc, flags, QUALITY_FILMSCAN1, N, 0); theirs = Batch(W, H, fmt, enc, flags, QUALITY_FILMSCAN1, N, 0, entry="ex")
    try:
        assert theirs.stats()[0] == -1
        for k in range(2):
            for bt in (mine, theirs): bt.feed(frames[k * N: (k + 1) * N])
            assert mine.roundtrip() == theirs.roundtrip()
            Q.assert_samples_equal(mine.samples(), theirs.samples(), "%s pass %d, create_stream against create_ex: " % (route, k))
            assert all(np.array_equal(a, b) for a, b in zip(mine.pictures(), theirs.pictures()))
            assert mine.stats() == (0, [1, N, 0]) and theirs.stats()[0] == -1
    finally:
        mine.close(); theirs.close()


# ------------------------------------------------------------------------------------------
# 4. the bit-rate limiter
# ------------------------------------------------------------------------------------------
LIMITER_N, LIMITER_PASSES = 6, 2
LIMITER_BOUND = {MEDIUM: 130000000, HIGH: 150000000}      # bits a second at the limiter's 30 fps (cfhd_tables.cpp limit_bitrate)
# The smallest geometry found, with the reference encoder on the CPU, whose noisy samples pass 1.2 x the bound at BOTH words: 1360 x 768.  Tried, by area, on frames of
# about 16:9 with sides that are multiples of 16 (bytes of the three noisy samples, HIGH | MEDIUM; 1.2 x the bound is 750 000 | 650 000 bytes a frame):
#   1280 x 720   757 448, 885 296, 1 080 884 | 579 808 (too small), ...        1344 x 768   848 580, 991 692, 1 210 612 | 649 764 (too small), ...
#   1360 x 768   861 492, 1 006 004, 1 227 744 | 659 920, 774 136, 936 752     1920 x 1080  1 713 228, 1 996 124, 2 432 688 | 1 311 760, 1 535 344, 1 854 520
# (960 x 544 and below stay under HIGH's bound altogether.)  At 1360 x 768 frames 2 .. 7 carry the coarser tables -- four of them flat frames behind flat frames -- and
# frames 8 .. 11 the normal ones again, at both words.
LIMITER_GEOMETRY = (1360, 768)


def limiter_frames(w, h):
    """One flat frame, three of feedback_test_frames, eight flat ones."""
    flat = np.full(w * h * 2, 128, np.uint8)
    noisy = feedback_test_frames(w, h, 3)
    return [flat] + noisy + [flat] * 8


_limiter = {}


def limiter_stream(quality, w, h):
    key = (quality, w, h)
    if key not in _limiter:
        frames = limiter_frames(w, h)
        refs = ref_encode_frames(frames, w * 2, w, h, quality=quality)
        limiter_input_does_its_job(refs, quality)
        _limiter[key] = (frames, refs)
    return _limiter[key]


def limiter_input_does_its_job(refs, quality):
    """On the reference's samples: the noisy samples beyond 1.2 x the bound, at least two flat frames behind them still on the coarser tables (the hysteresis of
    overbitrate, not only the tables of the frame behind a large sample), the last frames on the normal tables again."""
    t = [sample_tables(s) for s in refs]
    normal = t[0]
    for i in (1, 2, 3): assert len(refs[i]) * 8 * 30 > 1.2 * LIMITER_BOUND[quality], "noisy sample %d: %d bytes" % (i, len(refs[i]))
    # frame 4 follows a large sample; frames 5, 6, .. follow flat (small) ones
    coarse = [i for i in range(5, len(t)) if t[i] != normal]
    assert len(coarse) >= 2, "flat frames behind flat frames that still carry the coarser tables: %s" % coarse
    assert t[-1] == normal and t[-2] == normal, "the stream does not come back to the normal tables"


def check_limiter(quality):
    """MEDIUM / HIGH on 1360 x 768 YUY2 (LIMITER_GEOMETRY says why that size): six frames a pass, two passes; the limiter trips inside pass 0 and lets go in pass 1."""
    w, h = LIMITER_GEOMETRY
    frames, refs = limiter_stream(quality, w, h)
    bt = Batch(w, h, "YUY2", "422", 0, quality, LIMITER_N, 1)
    try:
        passes = run_stream(bt, frames, LIMITER_PASSES, queued=True)
    finally:
        bt.close()
    mine = [s for p in passes for s in p[0]]
    handle = amd_encode_frames(frames, w * 2, w, h, quality=quality)
    Q.assert_samples_equal(mine, handle, "quality %d against this library's handle: " % quality)
    Q.assert_samples_equal(mine, refs, "quality %d against the reference: " % quality)
    assert any(p[1][0] >= 2 for p in passes), [p[1] for p in passes]


# ------------------------------------------------------------------------------------------
# 5. queue and gates
# ------------------------------------------------------------------------------------------
def check_queue():
    """Two stream batches in flight -- one fed through submit_host from a registered buffer --, waited for in order: each is its own handle's stream.  Between submit and
    wait the shared entry points answer with their error values."""
    L = lib()
    streams = [stream("YUY2-422", FILMSCAN2), stream("YUY2-422i", FILMSCAN3)]
    args = [("YUY2", "422", 0, FILMSCAN2), ("YUY2", "422", INTERLACED, FILMSCAN3)]
    handles = [amd_encode_frames(frames, pitch, W, H, PIX_YUY2, quality=a[3], flags=a[2]) for (frames, pitch, _), a in zip(streams, args)]
    pitch = W * 2
    host = np.zeros(N * pitch * H, np.uint8)
    assert L.cfhd_amd_register_host_buffer(host.ctypes.data_as(V), host.nbytes) == 0
    bts = [Batch(W, H, a[0], a[1], a[2], a[3], N, 1) for a in args]
    try:
        for k in range(PASSES):
            bts[0].feed(streams[0][0][k * N: (k + 1) * N])
            host[:] = np.concatenate(streams[1][0][k * N: (k + 1) * N])
            assert L.cfhd_amd_batch_submit(bts[0].b) == 0, amd_last_error()
            assert L.cfhd_amd_batch_submit_host(bts[1].b, host.ctypes.data_as(V), pitch * H, pitch, None, 0, 0) == 0, amd_last_error()
            for bt in bts:
                p = V(); sz = ctypes.c_size_t(); buf = np.zeros(pitch * H, np.uint8); dx = (ctypes.c_uint32 * 16)()
                assert L.cfhd_amd_batch_roundtrip(bt.b) == -1 and L.cfhd_amd_batch_submit(bt.b) == -1
                assert L.cfhd_amd_batch_submit_host(bt.b, buf.ctypes.data_as(V), 0, pitch, None, 0, 0) == -1
                assert L.cfhd_amd_batch_upload(bt.b, 0, buf.ctypes.data_as(V), pitch) == -1
                assert L.cfhd_amd_batch_get_sample(bt.b, 0, ctypes.byref(p), ctypes.byref(sz)) == -1
                assert L.cfhd_amd_batch_download_output(bt.b, 0, buf.ctypes.data_as(V), pitch) == -1
                assert L.cfhd_amd_batch_kernel_ms(bt.b, 0) == 0 and L.cfhd_amd_batch_dx_stats(bt.b, dx) == -1
                assert bt.stats()[0] == -1
            for j, bt in enumerate(bts):
                total = L.cfhd_amd_batch_wait(bt.b)
                s = bt.samples()
                assert total == sum(len(x) for x in s), (total, amd_last_error())
                Q.assert_samples_equal(s, handles[j][k * N: (k + 1) * N], "batch %d pass %d: " % (j, k))
                assert bt.stats()[0] == 0
            assert L.cfhd_amd_batch_wait(bts[0].b) == -1          # nothing in flight
        assert L.cfhd_amd_batch_kernel_name(bts[0].b, 0) != b"" and L.cfhd_amd_batch_kernel_ms(bts[0].b, 6) >= 0
    finally:
        for bt in bts: bt.close()
        L.cfhd_amd_unregister_host_buffer(host.ctypes.data_as(V))


def refused(*a):
    """The text of a refusal, False for a batch that was made."""
    L = lib()
    b = L.cfhd_amd_batch_create_stream(*a)
    if b: L.cfhd_amd_batch_destroy(b); return False
    text = amd_last_error()
    assert text, "refused without a text"
    return text


def check_gates():
    L = lib()
    yuy2 = fourcc("YUY2")
    assert "cfhd_amd_batch_create_groups" in refused(W, H, yuy2, ENCODED_YUV422, GOP, FILMSCAN2, N, 1, 1)
    assert "cfhd_amd_batch_create_groups" in refused(W, H, yuy2, ENCODED_YUV422, GOP, QUALITY_FILMSCAN1, N, 1, 1)
    assert refused(W, H, yuy2, ENCODED_YUV422, 0, FILMSCAN2, 0, 1, 1) and refused(W, H, yuy2, ENCODED_YUV422, 0, FILMSCAN2, -3, 1, 1)
    assert refused(W, H, yuy2, ENCODED_RGB444, 0, FILMSCAN2, N, 1, 1), "an encoded format CFHD_PrepareToEncode refuses for YUY2"
    assert refused(W, H, fourcc("BYR4"), ENCODED_BAYER, 0, FILMSCAN2, N, 1, 0), "Bayer batches are encode only"
    assert refused(W, H, yuy2, ENCODED_YUV422, 0, 0, N, 1, 1), "a quality word with a low byte of 0"
    assert not refused(W, H, yuy2, ENCODED_YUV422, 0, FILMSCAN2, N, 1, 1) and not refused(W, H, yuy2, ENCODED_YUV422, 0, FILMSCAN2, 1, 1, 0)
    # cfhd_amd_batch_create_ex keeps refusing the words whose tables move: callers probe with it
    for quality in (FILMSCAN2, FILMSCAN3):
        b = L.cfhd_amd_batch_create_ex(W, H, yuy2, ENCODED_YUV422, 0, quality, N, 1, 1)
        if b: L.cfhd_amd_batch_destroy(b)
        assert not b, quality
    assert L.cfhd_amd_batch_stream_stats(None, (ctypes.c_int * 3)()) == -1


def gates_under_host_entropy():
    """Child process body (CFHD_AMD_ENTROPY=host is read when a batch is made; kept to a process of its own as tests/decode_queue.py does)."""
    for quality in (FILMSCAN2, QUALITY_FILMSCAN1):
        text = refused(W, H, fourcc("YUY2"), ENCODED_YUV422, 0, quality, N, 1, 1)
        assert text and "CFHD_AMD_ENTROPY" in text, text
    print("HOST ENTROPY REFUSED")


def host_entropy_child(emulated):
    """Runs gates_under_host_entropy in a child process with CFHD_AMD_ENTROPY=host."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["CFHD_AMD_ENTROPY"] = "host"
    code = "import sys; sys.path.insert(0, %r); import cfhd_testlib as T, stream_batches as S\n" % os.path.dirname(os.path.abspath(__file__))
    code += "with T.emulated_product(): S.gates_under_host_entropy()\n" if emulated else "S.gates_under_host_entropy()\n"
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "HOST ENTROPY REFUSED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
