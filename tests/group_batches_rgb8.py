"""Batches of two-frame groups from 8-bit RGB (RG24 / BGRA / BGRa) on the frame queue -- cfhd_amd_batch_create_groups -- and the device coding of their subband 7
(k_ent_split_two_pass + two holes of code set 18 without peaks): the helpers and test bodies shared by tests/test_gpu_group_batches_rgb8.py (hardware) and
tests/test_group_batches_rgb8_emulated.py (the same functions inside cfhd_testlib.emulated_product()).

The anchor of every sample is the REFERENCE encoder: one reference handle fed the frames of two passes (+ one call that flushes the last P-frame sample), byte for
byte after mask_volatile_metadata, through reference_leg.  Pictures (mode 0) against CFHD_DecodeSample's of the same samples, within one dither step (the rule of
tests/group_decode_queue.py::check_foreign_dithered; the handle's pictures are pinned on the reference by tests/test_gpu_group_outputs.py).

Sizes of luma subband 7 (w[3] is a quarter of the channel each way; table-1 segments are 1024 coefficients): 192 x 96 -> 48 x 24 = 1152, two segments (chroma 576: one);
320 x 240 -> 80 x 60 = 4800, five; 336 x 252 (coded height 256) -> 84 x 64 at pitch 88, six, chroma width 42 at pitch 48; 640 x 480 -> 160 x 120 = 19 200, nineteen.

Not reachable from here, covered by reading: NULL for "a geometry the device group decoder does not take" (dev::DecGroupPlan::two_pass == 0 needs a band offset or
pitch that is no multiple of 8, which build_gop_plan never lays out), and the pass result -9 (no picture of test size reaches 80 % of the sample buffer).
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *
import group_batches as GB
import gop_input_frames

FOURCCS = GB.FOURCCS
BYTES = {"RG24": 3, "BGRA": 4, "BGRa": 4}
# (input, w, h, frames, flash pairs)
CASES = [("RG24", 192, 96, 4, False), ("BGRA", 320, 240, 4, True), ("BGRa", 336, 252, 6, False), ("RG24", 640, 480, 4, True), ("RG24", 192, 96, 70, False)]
ROUNDTRIP_CASES = CASES[:3]
HANDLE_CASES = [(name, w, h) for w, h in ((192, 96), (208, 104)) for name in ("RG24", "BGRA", "BGRa")]


def lib():
    L = GB.lib()
    if not getattr(L, "_group_batches_rgb8_declared", False):
        L.cfhd_amd_batch_create_groups.restype = ctypes.c_void_p
        L.cfhd_amd_batch_create_groups.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_int] * 4
        L._group_batches_rgb8_declared = True
    return L


def flash_frames(name, w, h, nframes):
    """Flash pairs: the difference between the two frames of a group ramps horizontally from full negative to full positive (its amplitude grows down the picture, so
    that the divided subband 7 passes through every value between its extremes), with a few columns where the two frames are equal interleaved -- zero runs in
    subband 7, one of them around 0.4 w (raster index 1024 of the 640 x 480 luma band lies in it).  Blue runs against red and green, so the chroma bands flash too."""
    n = BYTES[name]
    y, x = np.mgrid[0:h, 0:w]
    ramp = (2.0 * x / (w - 1) - 1.0) * (0.55 + 0.45 * y / (h - 1))
    equal = (np.abs(x - 0.4 * w) < 16) | (x % 64 < 6)
    out = []
    for g in range(nframes // 2):
        d = 255.0 * ramp * (1 if g % 2 == 0 else -1) * (1.0 - 0.07 * (g // 2))
        for f in (0, 1):
            comps = []
            for k in range(n):
                s = -1.0 if k == 0 else 1.0                  # (component 0: blue in all three layouts)
                v = 127.5 + (s * d / 2 if f else -s * d / 2)
                v = np.where(equal, 128.0, v)
                comps.append(np.full((h, w), 255, np.uint8) if k == 3 else np.clip(np.rint(v), 0, 255).astype(np.uint8))
            fr = np.stack(comps, axis=2).reshape(-1).copy()
            fr.setflags(write=False)
            out.append(fr)
    return out, w * n


_cases = {}


def case_frames(name, w, h, nframes, flash):
    return flash_frames(name, w, h, nframes) if flash else gop_input_frames.frames(name, w, h, nframes)


def case(name, w, h, nframes, flash, quality=QUALITY_FILMSCAN1):
    """(frames, pitch, the reference's stream of frames + frames + [frames[0]]: sequence header, then group and P-frame samples of two passes) -- computed once, shared."""
    key = (name, w, h, nframes, flash, quality)
    if key not in _cases:
        frames, pitch = case_frames(name, w, h, nframes, flash)
        fed = list(frames) + list(frames) + [frames[0]]
        refs = ref_encode_frames(fed, pitch, w, h, pixfmt=FOURCCS[name], quality=quality, flags=GB.GOP)
        check_input_does_its_job(name, w, h, flash, refs)
        _cases[key] = (frames, pitch, refs)
    return _cases[key]


def oracle_luma_subband7(sample, gp):
    """Luma subband 7 of a group sample as its two passes carry it -- the divided values, height x pitch -- by the ORACLE's bit-serial band decoder
    (oracle/cfhd_oracle_ent.c orc_decode_band_bits, code set 18, divisor 1) run over each pass.  (oracle_decode_group does not take a band coded in two passes: on these
    samples its walk stops at that band, "8 bands decoded".  The same oracle decodes the band here, pass by pass; the split at the BAND_SECONDPASS tag and the sum
    low + (high << 8) in 16 bits are Codec/decoder.c:12862 DecodeBand16sLossless.)"""
    O = oracle()
    O.orc_decode_band_bits.restype = ctypes.c_long
    O.orc_decode_band_bits.argtypes = [c_u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, c_i16p]
    import group_decode_queue as GQ
    lo, hi = [(lo, hi) for wavelet, band, encoding, lo, hi in GQ.group_bands(sample) if encoding == 5][0]      # (channel order: luma first)
    d = gp.w[(0, 3)]
    payload = np.frombuffer(sample[lo: hi], np.uint8).copy()
    def one_pass(buf):
        out = np.zeros(d["height"] * d["pitch"], np.int16)
        bits = O.orc_decode_band_bits(p8(buf), buf.size, d["width"], d["height"], d["pitch"], 1, 2, None, 0, 0, 0, p16(out))
        assert bits > 0, "oracle band decoder -> %d" % bits
        return out, (bits + 31) // 32 * 4
    low, used = one_pass(payload)
    assert bytes(payload[used: used + 4]) == b"\x00\x52\x00\x00", "no BAND_SECONDPASS tag behind the first pass"
    high, _ = one_pass(payload[used + 4:].copy())
    return (low.astype(np.int32) + (high.astype(np.int32) << 8)).astype(np.int16).astype(np.int32).reshape(d["height"], d["pitch"])


def check_input_does_its_job(name, w, h, flash, refs):
    """A CPU check of the input, on the REFERENCE's samples: luma subband 7 (divided by 32) of the flash cases holds every kind of value the two passes treat apart."""
    if not flash: return
    gp = GopPlan(w, h, pixkind=PIXKIND[name])
    bands = [oracle_luma_subband7(s, gp) for s in refs[1::2][:2]]
    v = np.concatenate([b.reshape(-1) for b in bands])
    assert ((v >= -255) & (v <= -251)).any(), "no value in -255 .. -251"
    assert (v < -255).any(), "no value below -255"
    assert ((v >= -250) & (v <= -1)).any(), "no value in -250 .. -1"
    assert ((v > 0) & ((v & 0xff) >= 251)).any(), "no positive value whose low byte is 251 .. 255"
    assert ((v != 0) & (v % 256 == 0)).any(), "no nonzero multiple of 256"
    if (w, h) == (640, 480):
        flat = bands[0].reshape(-1)                          # (rows at the band's pitch, pad columns included: the raster the coder walks)
        assert any(flat[m - 1] == 0 and flat[m] == 0 for m in range(1024, flat.size, 1024)), "no zero run crosses a multiple of 1024 coefficients"


def equals_reference(mine, refs, what):
    """The reference leg every case goes through: sizes and bytes (volatile metadata masked) of the whole stream."""
    def leg():
        if [len(s) for s in mine] != [len(s) for s in refs]: return "sizes differ: %s vs %s" % ([len(s) for s in mine][:6], [len(s) for s in refs][:6])
        for i, (a, b) in enumerate(zip(mine, refs)):
            if mask_volatile_metadata(a) != mask_volatile_metadata(b): return "sample %d differs from the reference" % i
        return True
    assert reference_leg(leg, 2, what), what


def picture_pitch(name, w):
    return BYTES[name] * w if name in BYTES else GB.picture_pitch(name, w)


class Batch(GB.Batch):
    """One batch of cfhd_amd_batch_create_groups with its frames in HBM."""
    def __init__(self, w, h, name, nframes, mode, frames, pitch, quality=QUALITY_FILMSCAN1, flags=0):
        self.L = lib(); self.w, self.h, self.name, self.n, self.mode = w, h, name, nframes, mode
        self.b = self.L.cfhd_amd_batch_create_groups(w, h, FOURCCS[name], flags, quality, nframes, 1, mode)
        assert self.b, "cfhd_amd_batch_create_groups -> NULL (%s)" % amd_last_error()
        self.frames, self.pitch = frames, pitch
        for i, f in enumerate(self.frames):
            assert self.L.cfhd_amd_batch_upload(self.b, i, np.asarray(f).ctypes.data_as(ctypes.c_void_p), self.pitch) == 0, amd_last_error()

    def pictures(self):
        pitch = picture_pitch(self.name, self.w); out = []
        for i in range(self.n):
            o = np.full(pitch * self.h, 7, np.uint8)
            assert self.L.cfhd_amd_batch_download_output(self.b, i, o.ctypes.data_as(ctypes.c_void_p), pitch) == 0, amd_last_error()
            out.append(o)
        return out


# ---- 1. samples
def check_samples(name, w, h, nframes, flash):
    frames, pitch, refs = case(name, w, h, nframes, flash)
    modes = (1, 0) if (name, w, h, nframes, flash) in ROUNDTRIP_CASES else (1,)
    for mode in modes:
        bt = Batch(w, h, name, nframes, mode, frames, pitch)
        try:
            rc, header = GB.sequence_header(bt.L, bt.b)
            assert rc == 0 and len(header) == 40
            mine = [header]
            for k in range(2):
                total = bt.roundtrip()
                s = bt.samples()
                assert total == sum(len(x) for x in s[0::2])
                assert all(len(x) == 24 for x in s[1::2])
                mine += s
        finally:
            bt.close()
        equals_reference(mine, refs, "group batches from 8-bit RGB: samples from %s %dx%d, mode %d" % (name, w, h, mode))


# ---- 2. the handle
def check_handle(name, w, h, quality=QUALITY_FILMSCAN1, nframes=4):
    frames, pitch = gop_input_frames.frames(name, w, h, nframes)
    fed = list(frames) + [frames[0]]
    refs = ref_encode_frames(fed, pitch, w, h, pixfmt=FOURCCS[name], quality=quality, flags=GB.GOP)
    with GB.device_entropy():
        strict = amd_encode_frames(fed, pitch, w, h, FOURCCS[name], quality=quality, flags=GB.GOP)      # (asserts that every call returns 0)
    equals_reference(strict, refs, "CFHD_EncodeSample, device entropy stage: groups from %s %dx%d quality %d" % (name, w, h, quality))
    old = os.environ.pop("CFHD_AMD_ENTROPY", None)
    try:
        default = amd_encode_frames(fed, pitch, w, h, FOURCCS[name], quality=quality, flags=GB.GOP)
    finally:
        if old is not None: os.environ["CFHD_AMD_ENTROPY"] = old
    assert [mask_volatile_metadata(s) for s in default] == [mask_volatile_metadata(s) for s in strict], "the default path writes other bytes than CFHD_AMD_ENTROPY=device"


# ---- 3. pictures
def check_pictures(name, w, h, nframes, flash):
    frames, pitch, _ = case(name, w, h, nframes, flash)
    bt = Batch(w, h, name, nframes, 0, frames, pitch)
    try:
        bt.roundtrip()
        samples, pictures = bt.samples(), bt.pictures()
    finally:
        bt.close()
    want, aw, ah, wpitch = GB.cabi_group_pictures(samples, name)
    assert (aw, ah, wpitch) == (w, h, picture_pitch(name, w))
    for i in range(nframes):
        d = np.abs(pictures[i].astype(np.int16) - want[i].astype(np.int16))
        assert d.max() <= 1, "frame %d: %d bytes further than one dither step from CFHD_DecodeSample's picture" % (i, int((d > 1).sum()))


# ---- 4. the queue
def check_queue():
    """Two batches in flight through submit / wait and one through submit_host with its pictures: the same samples and pictures, byte for byte, as synchronous passes
    with the same step numbers; between submit and wait every other entry point refuses the batch."""
    L = lib()
    L.cfhd_amd_set_clip_guid(bytes(range(16)))
    w, h, name, n = 192, 96, "RG24", 4
    frames, pitch = gop_input_frames.frames(name, w, h, 2 * n)
    sets = [frames[:n], frames[n:]]
    ppitch = picture_pitch(name, w)
    def synchronous(fs, passes):
        bt = Batch(w, h, name, n, 0, fs, pitch)
        try:
            out = []
            for _ in range(passes): bt.roundtrip(); out.append((bt.samples(), bt.pictures()))
            return out
        finally:
            bt.close()
    want = [synchronous(fs, 2) for fs in sets]
    queued = [Batch(w, h, name, n, 0, fs, pitch) for fs in sets]
    try:
        for step in range(2):
            for bt in queued: assert L.cfhd_amd_batch_submit(bt.b) == 0
            bt = queued[0]
            p = ctypes.c_void_p(); sz = ctypes.c_size_t(); buf = np.zeros(ppitch * h, np.uint8); stats = (ctypes.c_uint32 * 16)()
            assert L.cfhd_amd_batch_roundtrip(bt.b) == -1 and L.cfhd_amd_batch_submit(bt.b) == -1
            assert L.cfhd_amd_batch_submit_host(bt.b, buf.ctypes.data_as(ctypes.c_void_p), 0, pitch, None, 0, 0) == -1
            assert L.cfhd_amd_batch_upload(bt.b, 0, buf.ctypes.data_as(ctypes.c_void_p), pitch) == -1
            assert L.cfhd_amd_batch_get_sample(bt.b, 0, ctypes.byref(p), ctypes.byref(sz)) == -1
            assert GB.sequence_header(L, bt.b)[0] == -1
            assert L.cfhd_amd_batch_download_output(bt.b, 0, buf.ctypes.data_as(ctypes.c_void_p), ppitch) == -1
            assert L.cfhd_amd_batch_kernel_ms(bt.b, 0) == 0 and L.cfhd_amd_batch_kernel_name(bt.b, 0) == b"" and L.cfhd_amd_batch_dx_stats(bt.b, stats) == -1
            for k, bt in enumerate(queued):
                total = L.cfhd_amd_batch_wait(bt.b)
                s, pics = bt.samples(), bt.pictures()
                assert total == sum(len(x) for x in s[0::2])
                assert [mask_volatile_metadata(x) for x in s] == [mask_volatile_metadata(x) for x in want[k][step][0]], "batch %d step %d: samples" % (k, step)
                assert all(np.array_equal(a, b) for a, b in zip(pics, want[k][step][1])), "batch %d step %d: pictures" % (k, step)
            assert L.cfhd_amd_batch_wait(queued[0].b) == -1          # nothing in flight
    finally:
        for bt in queued: bt.close()
    # fed from host memory, pictures coming back: frames and pictures at their own strides with a gap between them
    fs = sets[0]
    stride = pitch * h + 256; pstride = ppitch * h + 256
    src = np.zeros(stride * n, np.uint8); dst = np.full(pstride * n, 9, np.uint8)
    for i, f in enumerate(fs): src[i * stride: i * stride + pitch * h] = np.asarray(f)
    b = L.cfhd_amd_batch_create_groups(w, h, FOURCCS[name], 0, QUALITY_FILMSCAN1, n, 1, 0)
    assert b
    try:
        for step in range(2):
            assert L.cfhd_amd_batch_submit_host(b, src.ctypes.data_as(ctypes.c_void_p), stride, pitch, dst.ctypes.data_as(ctypes.c_void_p), pstride, ppitch) == 0, amd_last_error()
            total = L.cfhd_amd_batch_wait(b)
            assert total == sum(len(x) for x in want[0][step][0][0::2]), total
            for i in range(n):
                assert np.array_equal(dst[i * pstride: i * pstride + ppitch * h], want[0][step][1][i]), "host-fed step %d picture %d" % (step, i)
                assert (dst[i * pstride + ppitch * h: (i + 1) * pstride] == 9).all()
            p = ctypes.c_void_p(); sz = ctypes.c_size_t()
            for i in range(n):
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                assert mask_volatile_metadata(ctypes.string_at(p, sz.value)) == mask_volatile_metadata(want[0][step][0][i]), "host-fed step %d sample %d" % (step, i)
    finally:
        L.cfhd_amd_batch_destroy(b)


# ---- 5. gates
def check_gates():
    L = lib()
    create = lambda w, h, name, flags, quality, n, mode: L.cfhd_amd_batch_create_groups(w, h, FOURCCS[name], flags, quality, n, 1, mode)
    def refused(*a):
        b = create(*a)
        if b: L.cfhd_amd_batch_destroy(b)
        return not b
    for name in ("RG24", "YUY2"):
        for mode in (0, 1):
            assert refused(320, 240, name, 0, QUALITY_FILMSCAN1, 3, mode), "odd frame count"
            assert refused(320, 240, name, 0, 5, 4, mode), "FILMSCAN2: the group tables follow the previous key sample"
            assert refused(200, 240, name, 0, QUALITY_FILMSCAN1, 4, mode), "width 200"
            assert not refused(320, 240, name, 0, QUALITY_FILMSCAN1, 4, mode), "%s, mode %d: refused" % (name, mode)
    for name in ("RG24", "BGRA", "BGRa", "v210"):
        for mode in (0, 1): assert refused(320, 240, name, GB.INTERLACED, QUALITY_FILMSCAN1, 4, mode), "interlaced groups: YUY2 / 2vuy only (%s)" % name
    assert not refused(320, 240, "YUY2", GB.INTERLACED, QUALITY_FILMSCAN1, 4, 1)
    for name in ("RG64", "a214"):
        assert refused(320, 240, name, 0, QUALITY_FILMSCAN1, 4, 0), name + " has no decoder output"
        assert not refused(320, 240, name, 0, QUALITY_FILMSCAN1, 4, 1), name + ", encode only: refused"
    old = os.environ.get("CFHD_AMD_ENTROPY")
    os.environ["CFHD_AMD_ENTROPY"] = "host"
    try:
        for name in ("RG24", "YUY2"):
            for mode in (0, 1): assert refused(320, 240, name, 0, QUALITY_FILMSCAN1, 4, mode), "host entropy"
    finally:
        if old is None: os.environ.pop("CFHD_AMD_ENTROPY")
        else: os.environ["CFHD_AMD_ENTROPY"] = old
    # cfhd_amd_batch_create_ex keeps its refusals: callers probe with it
    for name in ("RG24", "BGRA", "BGRa"):
        b = L.cfhd_amd_batch_create_ex(320, 240, FOURCCS[name], ENCODED_YUV422, GB.GOP, QUALITY_FILMSCAN1, 4, 1, 1)
        if b: L.cfhd_amd_batch_destroy(b)
        assert not b, name
    # one YUY2 case: the same samples as cfhd_amd_batch_create_ex's (the metadata's GUID pinned; its DATE / TIME strings, which follow the clock, masked)
    L.cfhd_amd_set_clip_guid(bytes(range(16)))
    w, h, n = 320, 240, 4
    frames, pitch = GB.case_frames(w, h, "YUY2", 0, n)
    mine = Batch(w, h, "YUY2", n, 1, frames, pitch); theirs = GB.Batch(w, h, "YUY2", 0, n, 1)
    try:
        ha, hb = GB.sequence_header(L, mine.b), GB.sequence_header(L, theirs.b)
        assert ha[0] == 0 and ha == hb
        for k in range(2):
            assert mine.roundtrip() == theirs.roundtrip()
            a, b = mine.samples(), theirs.samples()
            assert [mask_volatile_metadata(x) for x in a] == [mask_volatile_metadata(x) for x in b], "pass %d: the two constructors' samples differ" % k
    finally:
        mine.close(); theirs.close()
