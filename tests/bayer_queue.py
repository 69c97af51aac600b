"""Bayer samples on the two queues: cfhd_amd_decode_batch_create_bayer (batches of Bayer intra samples decoded to the BYR4 mosaic) and cfhd_amd_batch_create_bayer (the
frame queue's round trip BYR4 -> Bayer sample -> BYR4), and the fused last level behind them, k_inv_bayer_strip.  The helpers and test bodies shared by
tests/test_gpu_bayer_queue.py (hardware) and tests/test_bayer_queue_emulated.py (the same functions inside cfhd_testlib.emulated_product()).

Every picture is 16-bit without dither: every comparison is byte for byte.  The witness is never the code under test: it is ONE CFHD_DecodeSample handle of this
library fed the same samples (decode_queue.handle_pictures) -- the pair k_inv_packed16 + k_bayer_to_byr4, which a handle always runs and which
tests/test_oracle_vs_ref.py::test_reference_byr4_decode_of_bayer_equals_oracle pins on the reference decoder -- and, where oracle/_ref is built, the reference
decoder itself (ref_decode_sample).  CFHD_AMD_INVERSE is read at every launch: one process switches between the fused kernel (strip) and the pair (tile).

Mosaic sizes, the smallest at which the fused kernel can go wrong:
  1008 x 244   planes 504 x 122, level-1 band 252 wide: 63 blocks -- two segments a row, the neighbour exchange across the seam; w & 7 == 4: the tail columns start
               inside a block; coded height 128 against a display height of 122: the last strip leaves rows unwritten; four strips of 16 band rows
  192 x 96     band 48 x 24: one segment, a full and a short strip, w & 7 == 0
A Bayer geometry whose level-1 band width is no multiple of 4 does not exist: the encoder takes component planes of whole 8-column groups only
(cfhd_tables.cpp build_frame_plan: width % 8 of every channel), so every band is a multiple of 4 wide and its pitch a multiple of 8 -- the pair is reached through
CFHD_AMD_INVERSE=tile and through small launches, and the `tile` leg of every body covers it.
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import device_pictures as DP
import hostile_pictures
from decode_queue import FULL, HALF, V, use_emulated

SHAPES = [(1008, 244), (192, 96)]
SOURCES = ("ref", "amd")
BYR4, BYR5 = fourcc("BYR4"), fourcc("BYR5")
FUSED, PAIR = b"k_inv_bayer_strip", b"k_inv_packed16+k_bayer_to_byr4"
ROUTES = (("strip", FUSED), ("tile", PAIR))
NOISE, CHECKER = 2, 3              # the frames of a case that push the clamps


def lib():
    L = DP.lib()
    if not getattr(L, "_bayer_queue_declared", False):
        L.cfhd_amd_decode_batch_create_bayer.restype = V       # (on the parent commit: AttributeError, at the first lookup of a new entry point)
        L.cfhd_amd_decode_batch_create_bayer.argtypes = [V, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
        L.cfhd_amd_batch_create_bayer.restype = V
        L.cfhd_amd_batch_create_bayer.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_int] * 4
        L.cfhd_amd_batch_submit.argtypes = [V]
        L.cfhd_amd_batch_wait.restype = ctypes.c_longlong; L.cfhd_amd_batch_wait.argtypes = [V]
        L.cfhd_amd_batch_download_output.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_batch_kernel_name.restype = ctypes.c_char_p; L.cfhd_amd_batch_kernel_name.argtypes = [V, ctypes.c_int]
        L.cfhd_amd_batch_kernel_ms.restype = ctypes.c_float; L.cfhd_amd_batch_kernel_ms.argtypes = [V, ctypes.c_int]
        L._bayer_queue_declared = True
    return L


class inverse:
    """CFHD_AMD_INVERSE for the launches inside: strip (the fused kernel wherever the geometry allows) or tile (the pair)."""
    def __init__(self, mode): self.mode = mode
    def __enter__(self): self.old = os.environ.get("CFHD_AMD_INVERSE"); os.environ["CFHD_AMD_INVERSE"] = self.mode
    def __exit__(self, *a):
        if self.old is None: os.environ.pop("CFHD_AMD_INVERSE", None)
        else: os.environ["CFHD_AMD_INVERSE"] = self.old


class Queue(DQ.Queue):
    """One Bayer decode batch prepared on `first` (BYR4, full resolution)."""
    def __init__(self, first, n, out="BYR4", resolution=FULL):
        self.L = lib(); self.n = n
        fb = ctypes.create_string_buffer(first, len(first))
        self.b = self.L.cfhd_amd_decode_batch_create_bayer(fb, len(first), DQ.FOURCCS[out], resolution, n)
        assert self.b, "cfhd_amd_decode_batch_create_bayer -> NULL (%s)" % amd_last_error()
        w = ctypes.c_int(); h = ctypes.c_int(); rb = ctypes.c_int()
        assert self.L.cfhd_amd_decode_batch_geometry(self.b, ctypes.byref(w), ctypes.byref(h), ctypes.byref(rb)) == 0
        self.w, self.h, self.row_bytes = w.value, h.value, rb.value

    def last_level(self):
        return self.L.cfhd_amd_decode_batch_kernel_name(self.b, 6)


# ---- frames, samples and the witnesses: computed once, shared, read-only
_cache = {}


def mosaics(w, h):
    """Eight distinct mosaics (uint8 views of w x h 16-bit photosites): two synth_bayer seeds, a noise mosaic over the full 16-bit range (NOISE), the checker mosaic of
    hostile_pictures (CHECKER: 0 / 65535 photosites), four more synth_bayer seeds."""
    key = ("mosaics", w, h)
    if key not in _cache:
        m = [synth_bayer(w, h, 7), synth_bayer(w, h, 8), hostile_pictures.words16("noise", h, w), hostile_pictures.words16("checker", h, w)] + [synth_bayer(w, h, 9 + i) for i in range(4)]
        _cache[key] = [np.ascontiguousarray(x, np.uint16).reshape(-1).view(np.uint8).copy() for x in m]
    return _cache[key]


def samples_of(w, h, source):
    key = ("samples", w, h, source, bool(use_emulated()))
    if key not in _cache:
        encode = ref_encode_frames if source == "ref" else amd_encode_frames
        _cache[key] = encode(mosaics(w, h), w * 2, w, h, BYR4, ENCODED_BAYER)
        assert len(set(_cache[key])) == 8
    return _cache[key]


def witness(w, h, source):
    """([picture of sample i], (w, h, row bytes)) from one CFHD_DecodeSample handle of this library; every return code 0."""
    key = ("witness", w, h, source, bool(use_emulated()))
    if key not in _cache:
        res, geometry = DQ.handle_pictures(samples_of(w, h, source), "BYR4", FULL)
        assert [rc for rc, _ in res] == [0] * 8 and geometry == (w, h, 2 * w)
        _cache[key] = ([p for _, p in res], geometry)
    return _cache[key]


def clamp_bounds():
    """What the clamps leave in a picture, through the reference's linear-restore table (the oracle's restatement): table[0] for a word clamped at 0 (to16 and the
    recombination), table[65520 >> 2] for a green at to16's top (4095 << 4, difference word 0), table[65535 >> 2] for the recombination's top."""
    O = oracle()
    lut = np.zeros(16384, np.uint16)
    O.orc_byr4_linear_restore_curve(lut.ctypes.data_as(ctypes.c_void_p))
    return int(lut[0]), int(lut[65520 >> 2]), int(lut[65535 >> 2])


def assert_clamps_reached(pictures, what):
    """The two clamp pictures of a case between them show every bound.  Measured on the handle's pictures under the emulator, words at (0, to16's top, the
    recombination's top): the checker mosaic 9 216 / 0 / 0 at 192 x 96 and 122 976 / 0 / 0 at 1008 x 244 -- its R and B clamp at 0, its greens come back at 65 389
    at the most --, the noise mosaic 0 / 10 / 196 and 25 / 127 / 2 520: the upper bounds are the noise's, the lower the checker's."""
    words = np.concatenate([pictures[NOISE].view(np.uint16), pictures[CHECKER].view(np.uint16)])
    counts = [int((words == v).sum()) for v in clamp_bounds()]
    assert (pictures[CHECKER].view(np.uint16) == clamp_bounds()[0]).any() and all(counts), "%s: the clamp pictures miss a clamp bound %s: %s -- choose other pictures" % (what, clamp_bounds(), counts)


def _same(a, b, what):
    assert np.array_equal(a, b), "%s: %d bytes differ" % (what, int((a != b).sum()))


def reference_agrees(w, h, samples):
    """The reference decoder's BYR4 pictures of the samples (a few attempts each: its threaded decoder occasionally returns other greens for a whole frame on the
    first call of a process, tests/test_oracle_vs_ref.py)."""
    return lambda i, mine: any(np.array_equal(np.frombuffer(ref_decode_sample(samples[i], w, h, BYR4)[0].tobytes(), np.uint8)[: 2 * w * h], mine) for _ in range(6))


# ---- 1. fused = pair = handle (= reference)
def check_fused_equals_pair_equals_handle(w, h, source):
    samples = samples_of(w, h, source)
    want, geometry = witness(w, h, source)
    assert_clamps_reached(want, "%d x %d %s" % (w, h, source))
    q = Queue(samples[0], 8)
    try:
        assert (q.w, q.h, q.row_bytes) == geometry
        got = {}
        for mode, name in ROUTES:
            with inverse(mode):
                ret, status, pictures = q.decode(samples)
                assert ret == 8 and status == [0] * 8, (mode, ret, status, amd_last_error())
                assert q.last_level() == name, (mode, q.last_level())
            got[mode] = pictures
            for i in range(8): _same(pictures[i], want[i], "%s, sample %d against the handle" % (mode, i))
        for i in range(8): _same(got["strip"][i], got["tile"][i], "sample %d, fused against the pair" % i)
        assert_clamps_reached(got["strip"], "fused, %d x %d %s" % (w, h, source))
        if have_ref():
            agrees = reference_agrees(w, h, samples)
            for i in (0, NOISE, CHECKER): assert agrees(i, got["strip"][i]), "sample %d differs from the reference decoder's picture" % i
    finally:
        q.close()


# ---- 2. a short pass, delivered into device memory
def check_short_pass_and_delivery(w, h, source="amd"):
    samples = samples_of(w, h, source)
    want, _ = witness(w, h, source)
    q = Queue(samples[0], 8)
    try:
        with inverse("strip"):
            d = DP.Delivery(q, DP.PACKED, True, 8)
            assert d.pitch > q.row_bytes and d.stride > d.pitch * q.h
            d.set()
            ret, status = DP.run_pass(q, samples, count=3)
            assert (ret, status) == (3, [0] * 3) and q.last_level() == FUSED
            d.check(want[:3] + [None] * 5, "count = 3 of 8: pictures, padding, the pictures behind the count")
            for i, p in enumerate(q.pictures(3)): _same(p, want[i], "download_output(%d) beside device delivery" % i)
            assert_clamps_reached(want, "%d x %d" % (w, h))
            # the whole batch, the clamp pictures included, into the same memory
            ret, status = DP.run_pass(q, samples)
            assert ret == 8 and status == [0] * 8
            d.check(want, "count = 8")
            # a short pass of other samples on top: the pictures behind its count are the full pass's still, in the caller's memory and in the batch's own -- the
            # last strip of picture 2 (coded rows beyond the display height) wrote nothing into picture 3
            ret, status = DP.run_pass(q, samples[5:8])
            assert (ret, status) == (3, [0] * 3)
            d.check(want[5:8] + [None] * 5, "count = 3 behind a full pass")
            for i, p in enumerate(q.pictures(8)): _same(p, (want[5:8] + want[3:])[i], "download_output(%d) behind a short pass" % i)
    finally:
        q.close()


# ---- 3. verdicts
def damaged_stream(sample, salt=0):
    """The sample with 64 bytes of a pattern in the middle of its longest coded band."""
    s = bytearray(sample)
    bands = DQ.walk_bands(sample)
    assert len(bands) == 36
    _, lo, hi = max(bands, key=lambda b: b[2] - b[1])
    at = (lo + (hi - lo) // 2) & ~3
    s[at: at + 64] = bytes((i * 37 + 11 + salt) & 0xff for i in range(64))
    return bytes(s)


def check_verdicts(w, h, source="amd"):
    good = samples_of(w, h, source)
    ow, oh = (192, 96) if (w, h) != (192, 96) else (208, 104)
    other = amd_encode_frames([synth_bayer(ow, oh, 5).reshape(-1).view(np.uint8).copy()], ow * 2, ow, oh, BYR4, ENCODED_BAYER)[0]
    yuv = DQ.samples_of("422", 192, 96, "amd", n=2)[0]
    samples = [good[0], good[1], damaged_stream(good[NOISE]), other, yuv, good[5]]
    sizes = [len(s) for s in samples]; sizes[1] = (len(good[1]) // 2) & ~3
    res, _ = DQ.handle_pictures(samples, "BYR4", FULL, sizes=sizes)
    want_status, want = [rc for rc, _ in res], [p for _, p in res]
    print("the handle answers", want_status)
    assert want_status[0] == 0 and want_status[5] == 0 and all(want_status[1:5]), "the damaged sample still decodes on the handle (%s): choose another pattern" % want_status
    q = Queue(good[0], 8)
    try:
        for mode, name in ROUTES:
            with inverse(mode):
                blob, offsets, _ = DQ.pack(samples)
                assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
                ret, status = q.wait(len(samples))
                pictures = q.pictures(len(samples))
                assert status == want_status and ret == status.count(0), (mode, status, want_status)
                for i in range(len(samples)):
                    _same(pictures[i], want[i], "%s: sample %d" % (mode, i))
                    if status[i]: assert not pictures[i].any(), "%s: sample %d failed and its picture is not zero" % (mode, i)
                # an intact pass on the same batch afterwards
                ret, status, pictures = q.decode(good)
                assert ret == 8 and status == [0] * 8 and q.last_level() == name
                for i in range(8): _same(pictures[i], witness(w, h, source)[0][i], "%s: intact pass behind the verdicts, sample %d" % (mode, i))
    finally:
        q.close()


# ---- 4. gates
def check_gates():
    L = lib()
    w, h = 192, 96
    bayer = samples_of(w, h, "amd")
    yuv = DQ.samples_of("422", w, h, "amd", n=2)[0]

    def refused(sample, out, resolution, n):
        fb = ctypes.create_string_buffer(sample, len(sample))
        b = L.cfhd_amd_decode_batch_create_bayer(fb, len(sample), DQ.FOURCCS[out], resolution, n)
        if b: L.cfhd_amd_decode_batch_destroy(b); return False
        text = amd_last_error()
        assert text, "refused without a text"
        return text
    assert "Bayer" in refused(yuv, "BYR4", FULL, 4), "a 4:2:2 first sample"
    assert refused(bayer[0], "RG48", FULL, 4), "output RG48"
    assert refused(bayer[0], "BYR4", HALF, 4), "half resolution"
    assert refused(bayer[0], "BYR4", DQ.QUARTER, 4), "quarter resolution"
    assert "nsamples" in refused(bayer[0], "BYR4", FULL, 0)
    # the old creator keeps its refusal and its text
    assert "Bayer samples are decoded by CFHD_DecodeSample" in DQ.refused(bayer[0], "BYR4", FULL, 4)
    # planar layouts on a Bayer batch
    q = Queue(bayer[0], 2)
    try:
        d = DP.Delivery(q, DP.PACKED, True, 2)
        for layout in (DP.PLANAR_U16, DP.PLANAR_F16, DP.PLANAR_F32):
            assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, d.mem.ptr + DP.GUARD, d.stride * 8, d.pitch * 2, layout) == -1
            assert "RG48" in amd_last_error()
        d.set()
    finally:
        q.close()

    def no_batch(*a):
        b = L.cfhd_amd_batch_create_bayer(*a)
        if b: L.cfhd_amd_batch_destroy(b); return False
        text = amd_last_error()
        assert text and "cfhd_amd_batch_create_bayer" in text, "refused without a text"
        return text
    assert "BYR5" in no_batch(w, h, BYR5, 0, QUALITY_FILMSCAN1, 4, 1, 0)
    assert no_batch(w, h, PIX_YUY2, 0, QUALITY_FILMSCAN1, 4, 1, 0) and no_batch(w, h, PIX_YUY2, 0, QUALITY_FILMSCAN1, 4, 1, 1)
    assert no_batch(w, h, BYR4, 0, 5, 4, 1, 0) and no_batch(w, h, BYR4, 0, 5, 4, 1, 1), "FILMSCAN2: tables that move"
    assert not no_batch(w, h, BYR5, 0, QUALITY_FILMSCAN1, 4, 1, 1) and not no_batch(w, h, BYR4, 0, QUALITY_FILMSCAN1, 4, 1, 0)
    # the old creators keep refusing mode 0 for Bayer
    b = L.cfhd_amd_batch_create_ex(w, h, BYR4, ENCODED_BAYER, 0, QUALITY_FILMSCAN1, 4, 1, 0)
    if b: L.cfhd_amd_batch_destroy(b)
    assert not b


# ---- 5. the frame queue's round trip
class Batch:
    def __init__(self, w, h, mode, n, entry="bayer"):
        self.L = L = lib(); self.n = n
        self.b = L.cfhd_amd_batch_create_bayer(w, h, BYR4, 0, QUALITY_FILMSCAN1, n, 1, mode) if entry == "bayer" else L.cfhd_amd_batch_create_ex(w, h, BYR4, ENCODED_BAYER, 0, QUALITY_FILMSCAN1, n, 1, mode)
        assert self.b, "%s mode %d -> NULL (%s)" % (entry, mode, amd_last_error())

    def feed(self, frames, pitch):
        for i, f in enumerate(frames): assert self.L.cfhd_amd_batch_upload(self.b, i, f.ctypes.data_as(V), pitch) == 0, amd_last_error()

    def samples(self):
        out = []
        for i in range(self.n):
            p = V(); n = ctypes.c_size_t()
            assert self.L.cfhd_amd_batch_get_sample(self.b, i, ctypes.byref(p), ctypes.byref(n)) == 0
            out.append(ctypes.string_at(p, n.value))
        return out

    def close(self):
        if self.b: self.L.cfhd_amd_batch_destroy(self.b); self.b = None


def check_frame_queue_round_trip(w, h):
    L = lib()
    all_frames = mosaics(w, h)
    bts = [Batch(w, h, 0, 4), Batch(w, h, 1, 4), Batch(w, h, 1, 4, entry="ex")]
    try:
        with inverse("strip"):
            for k in range(2):
                frames = all_frames[4 * k: 4 * k + 4]
                for bt in bts: bt.feed(frames, w * 2)
                for bt in bts: assert L.cfhd_amd_batch_submit(bt.b) == 0, amd_last_error()      # three batches in flight
                sets = []
                for bt in bts:
                    total = L.cfhd_amd_batch_wait(bt.b)
                    s = bt.samples()
                    assert total == sum(len(x) for x in s), (total, amd_last_error())
                    sets.append([mask_volatile_metadata(x) for x in s])
                assert sets[0] == sets[1], "pass %d: the samples of mode 0 and mode 1 differ" % k
                assert sets[0] == sets[2], "pass %d: the samples differ from cfhd_amd_batch_create_ex's" % k
                mine = bts[0].samples(); first_pass = []
                res, geometry = DQ.handle_pictures(mine, "BYR4", FULL)
                assert geometry == (w, h, 2 * w)
                for i in range(4):
                    o = np.full(2 * w * h, 7, np.uint8)
                    assert L.cfhd_amd_batch_download_output(bts[0].b, i, o.ctypes.data_as(V), 2 * w) == 0, amd_last_error()
                    assert res[i][0] == 0
                    _same(o, res[i][1], "pass %d picture %d against the handle's decode of get_sample(%d)" % (k, i, i))
                    if k == 0: first_pass.append(o)
                if k == 0: assert_clamps_reached(first_pass, "round trip, %d x %d" % (w, h))
                assert L.cfhd_amd_batch_kernel_name(bts[0].b, 3) == FUSED and L.cfhd_amd_batch_kernel_name(bts[1].b, 3) == b""
                assert L.cfhd_amd_batch_kernel_name(bts[0].b, 0) == L.cfhd_amd_batch_kernel_name(bts[2].b, 0) != b""
                assert L.cfhd_amd_batch_kernel_ms(bts[0].b, 3) >= 0 and L.cfhd_amd_batch_kernel_ms(bts[0].b, 13) >= 0
        # the pair behind the same batch
        with inverse("tile"):
            bts[0].feed(all_frames[:4], w * 2)
            assert L.cfhd_amd_batch_submit(bts[0].b) == 0 and L.cfhd_amd_batch_wait(bts[0].b) > 0
            assert L.cfhd_amd_batch_kernel_name(bts[0].b, 3) == PAIR
            res, _ = DQ.handle_pictures(bts[0].samples(), "BYR4", FULL)
            for i in range(4):
                o = np.full(2 * w * h, 7, np.uint8)
                assert L.cfhd_amd_batch_download_output(bts[0].b, i, o.ctypes.data_as(V), 2 * w) == 0
                _same(o, res[i][1], "tile: picture %d" % i)
    finally:
        for bt in bts: bt.close()
