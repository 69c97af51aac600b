"""Packed 4:2:2 pictures (YUY2, 2vuy, YU64) as planar Y, Cb, Cr tensors in device memory, on both queues: cfhd_amd_decode_batch_set_device_pictures with
CFHD_AMD_PICTURES_YUV422_U8 / _U16 / _F16 / _F32 (k_dec_deliver_yuv422: a picture of W x H pixels as Y, H rows of W elements at the pitch, then Cb and Cr, H rows of
W/2 elements each at half the pitch -- the I422 convention) and cfhd_amd_batch_upload_device_planar with CFHD_AMD_FRAMES_YUV422_* on every frame batch whose pixel
format is one of the three (k_enc_collect_yuv422, the mirror image).  The helpers and test bodies shared by tests/test_gpu_yuv422_planes.py (hardware) and
tests/test_yuv422_planes_emulated.py (the same functions inside cfhd_testlib.emulated_product(), where a device pointer is a host pointer).

Every comparison is exact; the float layouts are compared as bit patterns.  The witnesses are independent of the two kernels: a delivered picture is held to
cfhd_amd_decode_batch_download_output of the same pass, de-interleaved by numpy (split), and YU64 pictures, which carry no dither, to ONE CFHD_DecodeSample handle as
well; collected frames to cfhd_amd_batch_download_frame; samples to those of a batch of the same kind fed the numpy-interleaved frames (pack) through
cfhd_amd_batch_upload.  The element rules in numpy, with the unit of the format's own word (255 or 65535):
    delivery:   U8 / U16 the word;  F32 w.astype(float32) * (float32(1) / float32(unit));  F16 that .astype(float16)
    collection: U8 / U16 the element;  F32 t = x * float32(unit), NaN to 0, clip to [0, unit], rint;  F16 .astype(float32), then the F32 rule
Device buffers are checked whole: filled with a pattern, guards in front and behind, and afterwards equal to the pattern with exactly the row bytes of the planes
replaced (deliveries) or byte for byte what they were (sources).

Shapes: 192 x 96 (12 lanes a row: a partial wave), 1008 x 122 (63 groups of 16; 122 rows are no multiple of the four waves of a workgroup), 1040 x 40 (65 groups of 16:
the lane loop of either kernel makes a second trip) and, for delivery, 2096 x 40 (65 groups of 32, the U8 layout's group, and 16 pixels behind them) and half
resolution of 208 x 96 samples: pictures of 104 x 48, whole groups and the groups of eight behind them, chroma rows of 52 elements.
Test infrastructure only."""
import ctypes, os, subprocess
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import group_decode_queue as GQ
import device_pictures as DP
import planar_frames as PF
from device_pictures import DeviceArray, pattern, GUARD
from decode_queue import use_emulated, V, FULL, HALF

PACKED = 0
YUV422_U8, YUV422_U16, YUV422_F16, YUV422_F32 = 7, 8, 9, 10
LAYOUT_NAMES = {YUV422_U8: "u8", YUV422_U16: "u16", YUV422_F16: "f16", YUV422_F32: "f32"}
ELEMENT = {YUV422_U8: 1, YUV422_U16: 2, YUV422_F16: 2, YUV422_F32: 4}
FORMATS = ["YUY2", "2vuy", "YU64"]
PIX = {"YUY2": PIX_YUY2, "2vuy": PIX_2VUY, "YU64": PIX_YU64}
UNIT = {"YUY2": 255, "2vuy": 255, "YU64": 65535}
# the positions of Y0, Y1, Cb, Cr among the four bytes (words) of a pair of pixels
ORDER = {"YUY2": (0, 2, 1, 3), "2vuy": (1, 3, 0, 2), "YU64": (0, 2, 3, 1)}
SHAPES = [(192, 96), (1008, 122)]
LONG = (1040, 40)
LONG32 = (2096, 40)
HALF_OF = (208, 96)
GEOMETRY_SHAPES = SHAPES + [LONG]
FILMSCAN2 = PF.FILMSCAN2
DELIVER, COLLECT = b"k_dec_deliver_yuv422", b"k_enc_collect_yuv422"


def lib():
    L = PF.lib()
    if not getattr(L, "_yuv422_planes_declared", False):
        L.cfhd_amd_batch_create.restype = V
        L.cfhd_amd_batch_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L._yuv422_planes_declared = True
    return L


def word(fmt): return np.uint16 if fmt == "YU64" else np.uint8
def native(fmt): return YUV422_U16 if fmt == "YU64" else YUV422_U8
def layouts_of(fmt): return [native(fmt), YUV422_F16, YUV422_F32]
def row_bytes(fmt, w): return w * 2 * np.dtype(word(fmt)).itemsize


# ---- the two views of a picture, and the element rules
def split(picture, w, h, fmt):
    """A packed picture -> (Y [h, w], C [2, h, w/2]: Cb, Cr) in the format's own word."""
    quads = np.ascontiguousarray(picture).reshape(-1).view(word(fmt)).reshape(h, w // 2, 4)
    y0, y1, cb, cr = ORDER[fmt]
    return np.ascontiguousarray(quads[:, :, [y0, y1]]).reshape(h, w), np.ascontiguousarray(np.stack([quads[:, :, cb], quads[:, :, cr]]))


def pack(Y, C, fmt):
    """(Y [h, w], C [2, h, w/2]) -> the packed frame, uint8 [h, row bytes]."""
    h, w = Y.shape
    quads = np.empty((h, w // 2, 4), word(fmt))
    y0, y1, cb, cr = ORDER[fmt]
    quads[:, :, y0], quads[:, :, y1], quads[:, :, cb], quads[:, :, cr] = Y[:, 0::2], Y[:, 1::2], C[0], C[1]
    return quads.reshape(h, 2 * w).view(np.uint8)


def elements(words, layout, unit):
    """Words [..., n] -> the elements of `layout` by the delivery rule, uint8 [..., n * element size]."""
    words = np.ascontiguousarray(words)
    if layout in (YUV422_U8, YUV422_U16):
        assert words.dtype == (np.uint8 if layout == YUV422_U8 else np.uint16)
        return words.view(np.uint8)
    f32 = words.astype(np.float32) * (np.float32(1) / np.float32(unit))
    assert f32.dtype == np.float32
    if layout == YUV422_F32: return np.ascontiguousarray(f32).view(np.uint8)
    return np.ascontiguousarray(f32.astype(np.float16)).view(np.uint8)


def collected_words(bytes_, layout, unit):
    """Elements (uint8 [..., row bytes]) -> the words the collection rule gives, [..., n] in the word of the unit."""
    out = np.uint8 if unit == 255 else np.uint16
    b = np.ascontiguousarray(bytes_)
    if layout == YUV422_U8: assert unit == 255; return b.view(np.uint8)
    if layout == YUV422_U16: assert unit == 65535; return b.view(np.uint16)
    x = b.view(np.float16).astype(np.float32) if layout == YUV422_F16 else b.view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = x * np.float32(unit)
        assert t.dtype == np.float32
        t = np.where(np.isnan(t), np.float32(0), t)
        return np.rint(np.clip(t, np.float32(0), np.float32(unit))).astype(out)


def planes_of(picture, w, h, fmt, layout):
    """The planes of a packed picture in the element type of `layout` by the delivery rule: (Y uint8 [h, w * E], C uint8 [2, h, (w/2) * E])."""
    Y, C = split(picture, w, h, fmt)
    return elements(Y, layout, UNIT[fmt]), elements(C, layout, UNIT[fmt])


def collected(planes, fmt, layout):
    """(Y, C) of elements -> the packed frame the collection rule gives, uint8 [h, row bytes]."""
    return pack(collected_words(planes[0], layout, UNIT[fmt]), collected_words(planes[1], layout, UNIT[fmt]), fmt)


def geometry(w, h, layout, padded):
    """(luma row bytes, pitch, stride): the pitch the row bytes rounded up to 32 -- where they are a multiple of 32 the contiguous picture of 2 * h * pitch bytes --, or
    that + 64 and a stride of + 4096."""
    row = w * ELEMENT[layout]
    pitch = ((row + 31) & ~31) + (64 if padded else 0)
    return row, pitch, 2 * h * pitch + (4096 if padded else 0)


def place(image, at, pitch, h, row, planes):
    """The planes of one picture where the layout puts them in a buffer image: Y at `at`, Cb at at + h * pitch, Cr h * pitch / 2 further."""
    Y, C = planes
    image[at: at + h * pitch].reshape(h, pitch)[:, :row] = np.asarray(Y).reshape(h, row)
    image[at + h * pitch: at + 2 * h * pitch].reshape(2 * h, pitch // 2)[:, : row // 2] = np.asarray(C).reshape(2 * h, row // 2)


class Delivery(DP.Delivery):
    """device_pictures.Delivery for the three planes of the pictures of a 4:2:2 decode batch."""
    def __init__(self, q, fmt, layout, padded, npictures):
        self.q, self.fmt, self.layout = q, fmt, layout
        self.row, self.pitch, self.stride = geometry(q.w, q.h, layout, padded)
        self.image = pattern(GUARD + npictures * self.stride + GUARD)
        self.mem = DeviceArray(self.image)

    def expect(self, pictures):
        for i, p in enumerate(pictures):
            if p is not None: place(self.image, GUARD + i * self.stride, self.pitch, self.q.h, self.row, planes_of(p, self.q.w, self.q.h, self.fmt, self.layout))
        return self.image


class Source(PF.Source):
    """planar_frames.Source for frames of three planes ((Y, C) of elements) of w x h pictures."""
    def __init__(self, frames, w, h, layout, padded):
        self.w, self.h, self.layout, self.n = w, h, layout, len(frames)
        self.row, self.pitch, self.stride = geometry(w, h, layout, padded)
        self.image = pattern(GUARD + self.n * self.stride + GUARD)
        for i, f in enumerate(frames): place(self.image, GUARD + i * self.stride, self.pitch, h, self.row, f)
        self.mem = DeviceArray(self.image)


class Batch(PF.Batch):
    """planar_frames.Batch with cfhd_amd_batch_create among the constructors.  kind: (entry, pixel format, encoded format, flags, quality)."""
    def __init__(self, kind, w, h, n, mode=1):
        lib()
        if kind[0] != "create": PF.Batch.__init__(self, kind, w, h, n, mode); return
        self.L = L = lib(); self.w, self.h, self.n, self.mode = w, h, n, 0
        L.cfhd_amd_set_clip_guid(DP.GUID)
        self.b = L.cfhd_amd_batch_create(w, h, kind[1], kind[4], n, 1)
        assert self.b, "cfhd_amd_batch_create -> NULL (%s)" % amd_last_error()


def intra(fmt, flags=0): return ("ex", PIX[fmt], ENCODED_YUV422, flags, QUALITY_FILMSCAN1)


def compare_frame(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if np.array_equal(got, want): return
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    raise AssertionError("%s: %d of %d bytes differ, first at byte %d: %d, expected %d" % (what, bad.size, got.size, int(bad[0]), int(got.reshape(-1)[bad[0]]), int(want.reshape(-1)[bad[0]])))


# ---- frames for the frame queue: (Y, C) words of a format, textured, all different
def frame_words(fmt, w, h, i):
    """Frame i as (Y [h, w], C [2, h, w/2]) in the format's word: the textured YUY2 frame of the decode queue suites; for YU64 its bytes with low bytes of their own."""
    Y, C = split(np.ascontiguousarray(DQ._yuy2_frame(w, h, i, False)), w, h, "YUY2")
    if fmt != "YU64": return Y, C
    def widen(a, k): return (a.astype(np.uint16) << 8) | ((np.arange(a.size, dtype=np.uint32).reshape(a.shape) * 40503 + k) & 0xff).astype(np.uint16)
    return widen(Y, 3 + i), widen(C, 101 + i)


def packed_frames(fmt, w, h, n=4):
    return [pack(*frame_words(fmt, w, h, i), fmt) for i in range(n)]


# ---- 1. delivery equals numpy on download_output of the same pass
_interlaced = {}


def case_samples(kind, w, h):
    if kind == "422i":                                          # interlaced intra samples of textured frames (the field-flicker frames of decode_queue.samples_of are one picture at half resolution)
        key = (w, h, bool(use_emulated()))
        if key not in _interlaced: _interlaced[key] = amd_encode_frames([np.ascontiguousarray(synth_yuy2(w, h, 20 + i)[0]) for i in range(8)], w * 2, w, h, PIX_YUY2, ENCODED_YUV422, QUALITY_FILMSCAN1, 1)
        return _interlaced[key]
    if kind == "groups": return GQ.group_stream("amd" if (w, h) != SHAPES[0] else DP.source(), w, h, 0)
    if kind == "groups-i": return DP.interlaced_group_stream(w, h)
    return DQ.samples_of(kind, w, h, DP.source() if (w, h) == SHAPES[0] else "amd")


def case_queue(kind, samples, fmt, resolution):
    return GQ.GroupQueue(samples[0], fmt, resolution, 4) if kind.startswith("groups") else DQ.Queue(samples[0], fmt, resolution, 8)


def check_delivery(kind, w, h, fmt, resolution):
    """Every layout the format admits, into the tight geometry and into a pitch of + 64 with a stride of + 4096, on one batch: the layout is switched between passes."""
    samples = case_samples(kind, w, h)
    q = case_queue(kind, samples, fmt, resolution)
    L = lib()
    try:
        assert (q.w, q.h) == ((w, h) if resolution == FULL else (w // 2, h // 2)) and q.row_bytes == row_bytes(fmt, q.w)
        if (w, h) == LONG: assert q.w // 16 == 65               # (a lane of k_dec_deliver_yuv422 makes a second trip at 16 and at 8 pixels a lane)
        if (w, h) == LONG32: assert q.w // 32 == 65 and q.w % 32 == 16      # (... at 32 pixels a lane, the U8 layout's, and two groups of eight behind the last whole group)
        if (w, h) == HALF_OF: assert resolution == HALF and q.w % 16 == 8 and (q.w // 2) % 4 == 0      # (the half group behind the last whole one)
        handle = None
        if fmt == "YU64":                                       # no dither: the handle's pictures are the pass's
            res, geo = DQ.handle_pictures(samples, fmt, resolution)
            assert [rc for rc, _ in res] == [0] * 8 and geo == (q.w, q.h, q.row_bytes)
            handle = [p for _, p in res]
        for layout in layouts_of(fmt):
            for padded in (False, True):
                what = "%s %s %dx%d, %s, %s" % (kind, fmt, q.w, q.h, LAYOUT_NAMES[layout], "pitch + 64, stride + 4096" if padded else "the smallest pitch")
                d = Delivery(q, fmt, layout, padded, 8)
                if not padded and d.row % 32 == 0: assert d.pitch == q.w * ELEMENT[layout] and d.stride == 2 * q.h * d.pitch      # a contiguous (8, 2 * H * W) tensor
                if padded: assert d.pitch == ((d.row + 31) & ~31) + 64 and d.stride == 2 * q.h * d.pitch + 4096
                d.set()
                assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
                ret, status = DP.run_pass(q, samples)
                assert ret == 8 and status == [0] * 8, (what, ret, status, amd_last_error())
                want = q.pictures(8)
                assert len(set(p.tobytes() for p in want)) == 8
                if handle is not None:
                    for i in range(8): assert np.array_equal(want[i], handle[i]), "%s: download_output(%d) differs from the handle's picture" % (what, i)
                d.check(want, what)
    finally:
        q.close()


# ---- 2. a short pass touches nothing else; switching to PACKED, to NULL and back, the name under index 9 each time
def check_short_pass_and_switching(fmt, layout):
    w, h = SHAPES[0]
    samples = case_samples("422", w, h)
    q = DQ.Queue(samples[0], fmt, FULL, 8)
    L = lib()
    try:
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        d = Delivery(q, fmt, layout, True, 8)
        assert d.pitch > d.row and d.stride > 2 * h * d.pitch
        d.set()
        ret, status = DP.run_pass(q, samples, count=3)
        assert (ret, status) == (3, [0] * 3)
        d.check(q.pictures(3) + [None] * 5, "count = 3 of 8: planes, padding, gaps, the pictures behind the count, the guards")
        # PACKED between passes: the planes' buffer is left alone
        packed = DP.Delivery(q, PACKED, True, 8); packed.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        ret, status = DP.run_pass(q, samples[5:8])
        assert (ret, status) == (3, [0] * 3)
        packed.check(q.pictures(3) + [None] * 5, "PACKED behind a YUV422 layout")
        d.check([None] * 8, "the planes while PACKED is set")
        # NULL: neither buffer is touched
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check([None] * 8, "the planes after set_device_pictures(NULL)"); packed.check([None] * 8, "the packed buffer after set_device_pictures(NULL)")
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        # another plane layout of the format, then the first again, the whole batch
        other = [l for l in layouts_of(fmt) if l != layout][0]
        d2 = Delivery(q, fmt, other, False, 8); d2.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d2.check(q.pictures(8), "%s behind NULL" % LAYOUT_NAMES[other])
        d.check([None] * 8, "the first buffer while another is set")
        d.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check(q.pictures(8), "count = 8 behind PACKED, NULL and %s" % LAYOUT_NAMES[other])
    finally:
        q.close()


# ---- 3. verdicts and the slow path
def check_verdicts(fmt, layout):
    """device_pictures.check_verdicts' pass -- a damaged code stream (every sample the parser passed goes through the handle inside wait), a size that is no multiple
    of 4 (the slow path's), a sample the parser refuses for good --: zeros (0.0) in all three planes where a sample failed, the picture download_output gives (the
    handle's) everywhere else; for YU64 that picture is held to a handle of the test's own too."""
    w, h = SHAPES[0]
    intact = case_samples("422", w, h)
    samples = list(intact)
    samples[2], size2 = DQ.damaged("payload pattern", samples[2], None)
    samples[6], size6 = DQ.damaged("frame width", samples[6], None)
    sizes = [len(s) for s in samples]; sizes[2] = size2; sizes[6] = size6
    sizes[4] -= 2
    res, _ = DQ.handle_pictures(samples, fmt, FULL, sizes=sizes, first=intact[0])
    codes = [rc for rc, _ in res]
    print("the handle answers", codes)
    assert codes[6] != 0 and codes.count(0) >= 5
    q = DQ.Queue(intact[0], fmt, FULL, 8)
    try:
        d = Delivery(q, fmt, layout, True, 8); d.set()
        ret, status = DP.run_pass(q, samples, sizes)
        assert status == codes and ret == codes.count(0), (status, codes)
        got = q.pictures(8)
        for i, rc in enumerate(codes):
            if rc: assert not got[i].any(), "picture %d of a sample that failed is not zero" % i
            else: assert got[i].any()
            if fmt == "YU64": assert np.array_equal(got[i], res[i][1]), "picture %d differs from the handle's" % i
        d.check(got, "verdicts, %s %s" % (fmt, LAYOUT_NAMES[layout]))
        failed = codes.index(next(rc for rc in codes if rc))
        at = GUARD + failed * d.stride
        assert not d.mem.read()[at: at + h * d.pitch].reshape(h, d.pitch)[:, : d.row].any(), "the luma plane of a failed sample is 0 (0.0)"
        # an intact pass on the same batch and buffer afterwards
        ret, status = DP.run_pass(q, intact)
        assert ret == 8 and status == [0] * 8
        d.check(q.pictures(8), "an intact pass behind the damaged one")
    finally:
        q.close()


# ---- 4. collection equals numpy
RULE_W, RULE_H, RULE_N = 192, 96, 2
RULE_ELEMENTS = RULE_N * 2 * RULE_W * RULE_H                       # 73 728


def f32_rule_values(unit):
    """Singles for the F32 rule at a unit: for every k < unit the single nearest (k + 0.5) / unit and its two neighbours (among their products are the exact ties), 0.5
    itself, the specials -- zeros, infinities, NaNs, negatives, 1 and beyond, the smallest subnormal --, random 32-bit patterns for the rest."""
    k = np.arange(unit, dtype=np.float64)
    c = ((k + 0.5) / unit).astype(np.float32)
    near = np.stack([np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))], axis=1).reshape(-1)
    if unit == 65535:                                           # (196 605 of them: the exact ties alone, as tests/bayer_planes.py keeps them)
        prod = (near * np.float32(unit)).astype(np.float64)
        near = near[(prod - np.floor(prod)) == 0.5]
        assert near.size == 65537
    specials = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff], np.uint32).view(np.float32)
    more = np.array([0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.float32(1e-45), -1e30, 1e30, -0.25, 2.0], np.float32)
    rest = np.random.default_rng(22).integers(0, 1 << 32, RULE_ELEMENTS - near.size - specials.size - more.size, dtype=np.uint64).astype(np.uint32).view(np.float32)
    values = np.concatenate([near, specials, more, rest]).astype(np.float32)
    assert values.size == RULE_ELEMENTS
    return values


def rule_frames(fmt, layout):
    """Two frames of planes (73 728 elements).  U8: every byte; U16 and F16: i * 40503 mod 65536 over consecutive i -- every word, every binary16 pattern, its
    subnormals, infinities and NaNs among them; F32: f32_rule_values of the format's unit."""
    if layout == YUV422_U8: flat = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 37 + 11) & 0xff).astype(np.uint8)
    elif layout in (YUV422_U16, YUV422_F16):
        flat = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 40503) & 0xffff).astype(np.uint16)
        assert np.unique(flat).size == 65536
    else: flat = f32_rule_values(UNIT[fmt])
    per = flat.reshape(RULE_N, 2, RULE_H * RULE_W)
    E = ELEMENT[layout]
    return [(np.ascontiguousarray(per[i, 0]).view(np.uint8).reshape(RULE_H, RULE_W * E), np.ascontiguousarray(per[i, 1]).view(np.uint8).reshape(2, RULE_H, RULE_W // 2 * E)) for i in range(RULE_N)]


def check_collection(fmt, layout):
    w, h, n = RULE_W, RULE_H, RULE_N
    unit = UNIT[fmt]
    frames = rule_frames(fmt, layout)
    # what the rule says of the named values, whatever the frames hold
    one = lambda x, l: int(collected_words(np.array([x], np.float32 if l == YUV422_F32 else np.float16).view(np.uint8), l, unit)[0])
    for l in (YUV422_F16, YUV422_F32):
        assert one(0.5, l) == (128 if unit == 255 else 32768), "0.5: an exact tie, to even"
        assert one(np.nan, l) == 0 and one(-np.inf, l) == 0 and one(np.inf, l) == unit and one(-0.0, l) == 0 and one(-0.25, l) == 0 and one(1.0, l) == unit and one(2.0, l) == unit
    sub = collected_words(np.array([0x03ff, 0x0001], np.uint16).view(np.uint8), YUV422_F16, unit)      # binary16 subnormals: 1023 x 2^-24 and 2^-24
    assert list(sub) == ([0, 0] if unit == 255 else [4, 0])
    with Batch(intra(fmt), w, h, n) as bt:
        src = Source(frames, w, h, layout, False)
        assert src.pitch == w * ELEMENT[layout] and src.stride == 2 * h * src.pitch      # a contiguous (2, 2 * H * W) tensor
        src.feed(bt.L, bt.b, 0, n)
        for i in range(n): compare_frame(bt.frame(i, row_bytes(fmt, w)), collected(frames[i], fmt, layout), "%s %s, frame %d" % (fmt, LAYOUT_NAMES[layout], i))
        src.unchanged("%s %s" % (fmt, LAYOUT_NAMES[layout]))


# ---- 5. inversion
def all_words_pictures(fmt):
    """Two 192 x 96 pictures (73 728 words) that hold every byte -- every one of the 65 536 words -- of the format in luma and in chroma."""
    if fmt == "YU64": words = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 40503 + 977) & 0xffff).astype(np.uint16)
    else: words = np.random.default_rng(5).integers(0, 256, RULE_ELEMENTS).astype(np.uint8)
    pictures = list(words.view(np.uint8).reshape(RULE_N, RULE_H, row_bytes(fmt, RULE_W)))
    for p in pictures:
        Y, C = split(p, RULE_W, RULE_H, fmt)
        if fmt != "YU64": assert np.unique(Y).size == 256 and np.unique(C[0]).size == 256 and np.unique(C[1]).size == 256
    assert np.unique(words).size == UNIT[fmt] + 1
    return pictures


def check_inversion(fmt, layout):
    """collect(deliver(w)) = w: for the 8-bit unit through U8, F32 and F16 alike, for the 16-bit unit through U16 and F32; through F16 at the 16-bit unit, delivering
    what was collected returns every delivered bit pattern."""
    w, h, n = RULE_W, RULE_H, RULE_N
    pictures = all_words_pictures(fmt)
    planes = [planes_of(p, w, h, fmt, layout) for p in pictures]
    exact = not (fmt == "YU64" and layout == YUV422_F16)
    if layout == YUV422_F16 and fmt != "YU64":
        halves = elements(np.arange(256, dtype=np.uint8), YUV422_F16, 255).view(np.float16)
        assert np.unique(halves).size == 256 and np.abs(halves.astype(np.float64) * 255 - np.arange(256)).max() < 0.063
    with Batch(intra(fmt), w, h, n) as bt:
        src = Source(planes, w, h, layout, False)
        src.feed(bt.L, bt.b, 0, n)
        for i in range(n):
            got = bt.frame(i, row_bytes(fmt, w))
            if exact: compare_frame(got, pictures[i], "%s %s of the delivered picture %d" % (fmt, LAYOUT_NAMES[layout], i))
            else:
                again = planes_of(got, w, h, fmt, layout)
                assert np.array_equal(again[0], planes[i][0]) and np.array_equal(again[1], planes[i][1]), "f16: picture %d delivered, collected and delivered again" % i


# ---- 6. runs and geometry
def geometry_frames(fmt, w, h, layout):
    return [(elements(Y, layout, UNIT[fmt]), elements(C, layout, UNIT[fmt])) for Y, C in (frame_words(fmt, w, h, i) for i in range(4))]


def check_runs(fmt, w, h, layout):
    frames = geometry_frames(fmt, w, h, layout)
    want = [collected(f, fmt, layout) for f in frames]
    row = row_bytes(fmt, w)
    assert len(set(x.tobytes() for x in want)) == 4
    if (w, h) == LONG: assert w // 16 == 65
    for padded in (False, True):
        what = "%s %dx%d, %s, %s" % (fmt, w, h, LAYOUT_NAMES[layout], "pitch + 64, stride + 4096" if padded else "the smallest pitch")
        src = Source(frames, w, h, layout, padded)
        if not padded:
            with Batch(intra(fmt), w, h, 4) as bt:
                for first, count in ((1, 2), (0, 1), (3, 1)): src.feed(bt.L, bt.b, first, count)
                for i in range(4): compare_frame(bt.frame(i, row), want[i], "%s, frame %d" % (what, i))
        # frames 1 - 2 alone, over frames cfhd_amd_batch_upload put there
        held = [np.ascontiguousarray(want[(i + 2) % 4][::-1]) for i in range(4)]
        with Batch(intra(fmt), w, h, 4) as bt:
            bt.upload(held, row)
            src.feed(bt.L, bt.b, 1, 2)
            for i in range(4): compare_frame(bt.frame(i, row), want[i] if i in (1, 2) else held[i], "%s, frames 1 - 2 over uploaded frames, frame %d" % (what, i))
        src.unchanged(what)


# ---- 7. every kind of frame batch
# name: (format, kind, mode, CFHD_AMD_CHUNK).  "chunks": an intra batch cut into chunks with streams of their own (frames 0 - 2 | 3), a run that crosses the cut is split
KINDS = {"create-yuy2": ("YUY2", ("create", PIX_YUY2, 0, 0, QUALITY_FILMSCAN1), 0, None),
         "ex-2vuy-mode1": ("2vuy", intra("2vuy"), 1, None), "ex-yu64-mode0": ("YU64", intra("YU64"), 0, None),
         "interlaced-yuy2-mode0": ("YUY2", intra("YUY2", 1), 0, None), "interlaced-2vuy-mode1": ("2vuy", intra("2vuy", 1), 1, None),
         "groups-yuy2": ("YUY2", ("groups", PIX_YUY2, 0, 0, QUALITY_FILMSCAN1), 1, None), "groups-yu64": ("YU64", ("groups", PIX_YU64, 0, 0, QUALITY_FILMSCAN1), 1, None),
         "stream-filmscan2-yuy2": ("YUY2", ("stream", PIX_YUY2, ENCODED_YUV422, 0, FILMSCAN2), 1, None),
         "group-stream-2vuy": ("2vuy", ("group_stream", PIX_2VUY, 0, 0, QUALITY_FILMSCAN1), 1, None),
         "chunks-yuy2": ("YUY2", intra("YUY2"), 1, "3")}
KIND_IDS = list(KINDS)
_host_fed = {}


class chunked:
    def __init__(self, value): self.value = value
    def __enter__(self):
        self.old = os.environ.get("CFHD_AMD_CHUNK")
        if self.value is not None: os.environ["CFHD_AMD_CHUNK"] = self.value
    def __exit__(self, *a):
        if self.value is None: return
        if self.old is None: os.environ.pop("CFHD_AMD_CHUNK", None)
        else: os.environ["CFHD_AMD_CHUNK"] = self.old


def host_fed(name, w, h, frames):
    key = (name, w, h, bool(use_emulated()))
    if key not in _host_fed:
        fmt, kind, mode, chunk = KINDS[name]
        with chunked(chunk), Batch(kind, w, h, 4, mode) as bt:
            bt.upload(frames, row_bytes(fmt, w))
            samples = bt.run()
            _host_fed[key] = (samples, bt.outputs(row_bytes(fmt, w)) if bt.mode == 0 else None)
    return _host_fed[key]


def check_kind(name, layout=None):
    w, h = SHAPES[0]
    fmt, kind, mode, chunk = KINDS[name]
    layout = native(fmt) if layout is None else layout
    row = row_bytes(fmt, w)
    words = [frame_words(fmt, w, h, i) for i in range(4)]
    frames = [pack(Y, C, fmt) for Y, C in words]
    if "filmscan2" in name: assert lib().cfhd_amd_quantizer_is_static(w, h, PIX[fmt], ENCODED_YUV422, 0, FILMSCAN2) == 0, "the tables of this stream move"
    first, first_out = host_fed(name, w, h, frames)
    assert len(set(first)) == 4 or "group" in name             # (groups: two group samples, two 24-byte P-frame samples)
    src = Source([(elements(Y, layout, UNIT[fmt]), elements(C, layout, UNIT[fmt])) for Y, C in words], w, h, layout, True)
    with chunked(chunk), Batch(kind, w, h, 4, mode) as bt:
        assert bt.L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT
        if chunk: src.feed(bt.L, bt.b, 1, 3); src.feed(bt.L, bt.b, 0, 1)
        else: src.feed(bt.L, bt.b, 0, 4)
        for i in range(4): compare_frame(bt.frame(i, row), frames[i], "%s: frame %d in front of the pass" % (name, i))
        second = bt.run()
        if "filmscan2" in name:
            stats = (ctypes.c_int * 3)()
            assert bt.L.cfhd_amd_batch_stream_stats(bt.b, stats) == 0
            print("%s: %d rounds, %d frames coded, %d units whose tables moved" % (name, stats[0], stats[1], stats[2]))
        for i in range(4): assert second[i] == first[i], "%s, %s: sample %d of the batch fed from planes differs (%d / %d bytes)" % (name, LAYOUT_NAMES[layout], i, len(second[i]), len(first[i]))
        if bt.mode == 0:
            # (8-bit outputs dither with a seed that follows the pass: the batch fed from planes ran one pass, as the host-fed one did)
            for i, o in enumerate(bt.outputs(row)): assert np.array_equal(o, first_out[i]), "%s, %s: picture %d of the batch fed from planes differs" % (name, LAYOUT_NAMES[layout], i)
        for i in range(4): compare_frame(bt.frame(i, row), frames[i], "%s: frame %d behind the pass" % (name, i))
    src.unchanged(name)


# ---- 8. the chain, all in HBM: decode queue -> planes -> frame queue
def check_chain(fmt, layout):
    """Decode batch -> planes -> frame batch: cfhd_amd_batch_download_frame equals the decode's packed picture (download_output of the same pass)."""
    w, h = SHAPES[0]
    samples = case_samples("422", w, h)
    row = row_bytes(fmt, w)
    q = DQ.Queue(samples[0], fmt, FULL, 8)
    try:
        d = Delivery(q, fmt, layout, True, 8); d.set()
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        pictures = q.pictures(8)
        with Batch(intra(fmt), w, h, 8) as bt:
            assert bt.L.cfhd_amd_batch_upload_device_planar(bt.b, 0, 8, d.mem.ptr + GUARD, d.stride, d.pitch, layout) == 0, amd_last_error()
            for i in range(8): compare_frame(bt.frame(i, row), pictures[i].reshape(h, row), "%s %s: frame %d of the chain" % (fmt, LAYOUT_NAMES[layout], i))
            assert len(set(bt.run())) == 8
        d.check(pictures, "the delivered planes behind the frame queue's pass")
    finally:
        q.close()


# ---- 9. gates
def check_decode_gates():
    w, h = SHAPES[0]
    L = lib()
    yuv = case_samples("422", w, h)
    import bayer_queue as BQ
    queues = {"YUY2": DQ.Queue(yuv[0], "YUY2", FULL, 8), "YU64": DQ.Queue(yuv[0], "YU64", FULL, 2), "v210": DQ.Queue(yuv[0], "v210", FULL, 2), "RG48": DQ.Queue(yuv[0], "RG48", FULL, 2)}
    bayer = BQ.Queue(BQ.samples_of(w, h, "amd")[0], 2)
    try:
        q, yu64 = queues["YUY2"], queues["YU64"]
        d = Delivery(q, "YUY2", YUV422_F32, True, 8)
        p, stride, pitch = d.mem.ptr + GUARD, d.stride, d.pitch
        def refused(queue, ptr, s, pt, layout, what):
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, ptr, s, pt, layout) == -1, what
            text = amd_last_error()
            assert text and "decode queue" in text, "%s: refused without a text (%r)" % (what, text)
            return text
        # the refusals that must not move: layouts 4 .. 6 and -1 on a YU64 batch, and 7 on a Bayer batch, are unknown layouts; PLANAR_* on a YU64 batch names RG48
        unknown = set(refused(yu64, p, stride, pitch, layout, "layout %d on a YU64 batch" % layout) for layout in (4, 5, 6, -1, 11))
        unknown.add(refused(bayer, p, stride, pitch, 7, "layout 7 on a Bayer batch")); unknown.add(refused(bayer, p, stride, pitch, 10, "layout 10 on a Bayer batch"))
        assert len(unknown) == 1 and "unknown layout" in list(unknown)[0], unknown
        rgb = set(refused(yu64, p, stride, pitch, layout, "PLANAR layout %d on a YU64 batch" % layout) for layout in (1, 2, 3))
        assert len(rgb) == 1 and "RG48" in list(rgb)[0], rgb
        # the new refusals
        elsewhere = set(refused(queues[name], p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) for name in ("v210", "RG48") for layout in (7, 8, 9, 10))
        u8 = refused(yu64, p, stride, pitch, YUV422_U8, "U8 on a YU64 batch")
        u16 = refused(q, p, stride, pitch, YUV422_U16, "U16 on a YUY2 batch")
        off32 = set(refused(q, p, stride, pitch + 16, layout, "a pitch off 32, %s" % LAYOUT_NAMES[layout]) for layout in layouts_of("YUY2"))
        low_pitch = set(refused(q, p, stride, w * ELEMENT[layout] - 32, layout, "a pitch below W x element size, %s" % LAYOUT_NAMES[layout]) for layout in layouts_of("YUY2"))
        low_pitch.add(refused(q, p, stride, -pitch, YUV422_F32, "a negative pitch"))
        smallest = lambda pt, layout: h * pt + (2 * h - 1) * (pt // 2) + (w // 2) * ELEMENT[layout]
        low_stride = set(refused(q, p, smallest(pt, layout) - 16, pt, layout, "a stride below the three planes, %s" % LAYOUT_NAMES[layout])
                         for layout, pt in ((YUV422_U8, pitch), (YUV422_F16, w * 2), (YUV422_F32, pitch)))
        off = set([refused(q, p + 8, stride, pitch, YUV422_F32, "a pointer off 16"), refused(q, p, stride + 8, pitch, YUV422_F32, "a stride off 16"), refused(q, p, stride, pitch + 8, YUV422_F32, "a pitch off 16")])
        for s in (elsewhere, off32, low_pitch, low_stride, off): assert len(s) == 1, s
        assert len(unknown | rgb | elsewhere | {u8} | {u16} | off32 | low_pitch | low_stride | off) == 9, "the texts of the refusals are distinct"
        # the smallest pitch and stride are served
        for layout in layouts_of("YUY2"):
            row = w * ELEMENT[layout]
            assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, p, smallest(row, layout), row, layout) == 0, amd_last_error()
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, p, smallest(pitch, YUV422_F32), pitch, YUV422_F32) == 0, amd_last_error()
        assert L.cfhd_amd_decode_batch_set_device_pictures(yu64.b, p, smallest(w * 2, YUV422_U16), w * 2, YUV422_U16) == 0, amd_last_error()
        # a refusal leaves the layout that was set in place, and nothing was launched: the memory holds what was there
        refused(q, p, stride, w * 4 - 32, YUV422_F32, "a pitch below the row bytes, again")
        d.check([None] * 8, "behind refused calls")
        # a pass in flight refuses
        d.set()
        blob, offsets, sizes = DQ.pack(yuv)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        try:
            assert "flight" in refused(q, p, stride, pitch, YUV422_F32, "a pass in flight")
            assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == -1 and amd_last_error()
        finally:
            ret, status = q.wait(8)
        assert ret == 8 and status == [0] * 8
        d.check(q.pictures(8), "the pass the refused calls were made in")
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER and L.cfhd_amd_decode_batch_kernel_name(queues["RG48"].b, 9) == b"k_dec_deliver"
    finally:
        for x in queues.values(): x.close()
        bayer.close()


def check_frame_gates():
    w, h = SHAPES[0]
    L = lib()
    import bayer_planes as BP
    frames = geometry_frames("YUY2", w, h, YUV422_F32)
    src = Source(frames, w, h, YUV422_F32, True)
    p, stride, pitch = src.at(0), src.stride, src.pitch
    row = row_bytes("YUY2", w)
    def refused(b, first, count, ptr, s, pt, layout, what):
        assert L.cfhd_amd_batch_upload_device_planar(b, first, count, ptr, s, pt, layout) == -1, what
        text = amd_last_error()
        assert text and "planar" in text, "%s: refused without a text (%r)" % (what, text)
        return text
    # the refusals that must not move
    with BP.Batch(BP.EX, w, h, 4) as byr4:
        t_byr4 = set(refused(byr4.b, 0, 1, p, stride, pitch, layout, "layout %d on a BYR4 batch" % layout) for layout in (1, 0, 7, 8, 9, 10, -1))
    t_elsewhere = set()
    with Batch(PF.RG48_444, w, h, 4) as rg48:
        t_bayer_on_rgb = set(refused(rg48.b, 0, 1, p, stride, pitch, layout, "layout %d on an RG48 batch" % layout) for layout in (4, 5, 6))
        t_elsewhere |= set(refused(rg48.b, 0, 1, p, stride, pitch, layout, "layout %d on an RG48 batch" % layout) for layout in (7, 8, 9, 10))
    for name, pix in (("v210", PIX_V210), ("avu8", fourcc("avu8"))):
        with Batch(("ex", pix, ENCODED_YUV422, 0, QUALITY_FILMSCAN1), w, h, 4) as other:
            t_elsewhere |= set(refused(other.b, 0, 1, p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) for layout in (7, 9, 10))
    with Batch(intra("YU64"), w, h, 4) as yu64:
        t_u8 = refused(yu64.b, 0, 1, p, stride, pitch, YUV422_U8, "U8 on a YU64 batch")
    with Batch(intra("YUY2"), w, h, 4) as bt:
        b = bt.b
        assert "RG48" in refused(b, 0, 1, p, stride, pitch, 1, "PLANAR_U16 on a YUY2 batch")
        t_bayer = set(refused(b, 0, 1, p, stride, pitch, layout, "BAYER layout %d on a YUY2 batch" % layout) for layout in (4, 5, 6))
        assert len(t_bayer) == 1 and "BYR4" in list(t_bayer)[0] and len(t_bayer_on_rgb) == 1 and "unknown layout" in list(t_bayer_on_rgb)[0]
        t_u16 = refused(b, 0, 1, p, stride, pitch, YUV422_U16, "U16 on a YUY2 batch")
        t_off32 = set(refused(b, 0, 1, p, stride, pitch + 16, layout, "a pitch off 32, %s" % LAYOUT_NAMES[layout]) for layout in layouts_of("YUY2"))
        t_low = set(refused(b, 0, 1, p, stride, w * ELEMENT[layout] - 32, layout, "a pitch below W x element size, %s" % LAYOUT_NAMES[layout]) for layout in layouts_of("YUY2"))
        t_low.add(refused(b, 0, 1, p, stride, -pitch, YUV422_F32, "a negative pitch"))
        t_stride = set(refused(b, 0, 2, p, 2 * h * pt - 16, pt, layout, "a stride below the three planes, %s" % LAYOUT_NAMES[layout]) for layout, pt in ((YUV422_U8, pitch), (YUV422_F16, w * 2), (YUV422_F32, pitch)))
        t_off = set([refused(b, 0, 1, p + 8, stride, pitch, YUV422_F32, "a pointer off 16"), refused(b, 0, 2, p, stride + 8, pitch, YUV422_F32, "a stride off 16"), refused(b, 0, 1, p, stride, pitch + 8, YUV422_F32, "a pitch off 16")])
        t_run = set([refused(b, 0, 0, p, stride, pitch, YUV422_F32, "count 0"), refused(b, 3, 2, p, stride, pitch, YUV422_F32, "a run that leaves the batch"), refused(b, -1, 1, p, stride, pitch, YUV422_F32, "a run in front of the batch")])
        t_null = refused(b, 0, 1, None, stride, pitch, YUV422_F32, "no pointer")
        for s in (t_byr4, t_elsewhere, t_off32, t_low, t_stride, t_off, t_run): assert len(s) == 1, s
        assert len(t_byr4 | t_bayer | t_elsewhere | {t_u8} | {t_u16} | t_off32 | t_low | t_stride | t_off | t_run | {t_null}) == 11, "the texts of the refusals are distinct"
        # nothing was launched: the frames are what upload put there
        held = [np.ascontiguousarray(collected(f, "YUY2", YUV422_F32)[::-1]) for f in frames]
        bt.upload(held, row)
        refused(b, 0, 1, p, stride, w * 4 - 32, YUV422_F32, "a pitch below the f32 row bytes, again")
        for i in range(4): compare_frame(bt.frame(i, row), held[i], "behind refused calls, frame %d" % i)
        # the smallest pitch and stride are served
        tight = Source(frames, w, h, YUV422_F32, False)
        assert L.cfhd_amd_batch_upload_device_planar(b, 0, 4, tight.at(0), 2 * h * w * 4, w * 4, YUV422_F32) == 0, amd_last_error()
        # a pass in flight refuses
        assert L.cfhd_amd_batch_submit(b) == 0, amd_last_error()
        try:
            assert "flight" in refused(b, 0, 1, p, stride, pitch, YUV422_F32, "a pass in flight")
        finally:
            total = L.cfhd_amd_batch_wait(b)
        assert total > 0, (total, amd_last_error())
        want = [collected(f, "YUY2", YUV422_F32) for f in frames]
        for i in range(4): compare_frame(bt.frame(i, row), want[i], "behind the pass, frame %d" % i)
        tight.unchanged("gates, the tight source")
    src.unchanged("gates")


# ---- 10. the host statement of the rules
RULES_PROGRAM = r"""
// the element rules of cfhd_deliver_kernels.h and cfhd_collect_kernels.h at both units as a host compiler builds them:
//   "d <unit> <word> <f32 bits> <f16 bits>" for every word of the unit, "h <unit> <binary16 pattern> <word>" for all 65 536 patterns,
//   "f <unit> <single's bits> <word>" for every 32-bit pattern of the file named on the command line
#include "hip_emu.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
#include "cfhd_deliver_kernels.h"
#include "cfhd_collect_kernels.h"
#include <stdio.h>
#include <vector>
using namespace cfhd::dev;
template <int UNIT> void rules(const std::vector<unsigned> &bits)
{
	for (unsigned w = 0; w <= (unsigned)UNIT; w++) { const float f = deliver_unit_f32_of<UNIT>(w); unsigned b; memcpy(&b, &f, 4); printf("d %d %u %u %u\n", UNIT, w, b, deliver_f16_bits(f)); }
	for (unsigned h = 0; h < 65536u; h++) printf("h %d %u %u\n", UNIT, h, collect_word_f16_of<UNIT>(h));
	for (unsigned b : bits) { float x; memcpy(&x, &b, 4); printf("f %d %u %u\n", UNIT, b, collect_word_f32_of<UNIT>(x)); }
}
int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 3;
	std::vector<unsigned> bits(1 << 18);
	bits.resize(fread(bits.data(), 4, bits.size(), f));
	fclose(f);
	rules<255>(bits); rules<65535>(bits);
	return 0;
}
"""


def check_host_statement():
    """All 256 bytes and all 65 536 words through the host-compiled delivery rules, all binary16 patterns and the float32 sets of check_collection through the
    collection rules, both units, against numpy; and the inversion property of the 8-bit unit, the F16 leg included, on the program's own numbers."""
    build = os.path.join(ROOT, "tests", "_build"); os.makedirs(build, exist_ok=True)
    src, exe, data = os.path.join(build, "yuv422_rules.cpp"), os.path.join(build, "yuv422_rules"), os.path.join(build, "yuv422_rules_f32.bin")
    headers = [os.path.join(PRODUCT_DIR, "csrc", f) for f in ("cfhd_deliver_kernels.h", "cfhd_collect_kernels.h")]
    if not os.path.exists(src) or open(src).read() != RULES_PROGRAM: open(src, "w").write(RULES_PROGRAM)
    DP.cfhd_testlib_build_once(exe, ["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hipemu"), "-I" + os.path.join(PRODUCT_DIR, "csrc"), src], [src] + headers)
    values = np.concatenate([f32_rule_values(255), f32_rule_values(65535)])
    values.view(np.uint32).tofile(data)
    lines = subprocess.run([exe, data], capture_output=True, text=True, check=True, timeout=300).stdout.split("\n")
    for unit in (255, 65535):
        tag = " %d " % unit
        rows = lambda c: np.array([[int(x) for x in line.split()[2:]] for line in lines if line.startswith(c + tag)], dtype=np.uint32)
        d, hh, ff = rows("d"), rows("h"), rows("f")
        words = np.arange(unit + 1, dtype=np.uint8 if unit == 255 else np.uint16)
        assert d.shape == (unit + 1, 3) and np.array_equal(d[:, 0], words)
        assert np.array_equal(d[:, 1], elements(words, YUV422_F32, unit).view(np.uint32)), "the f32 delivery rule at unit %d" % unit
        assert np.array_equal(d[:, 2], elements(words, YUV422_F16, unit).view(np.uint16)), "the f16 delivery rule at unit %d" % unit
        assert hh.shape == (65536, 2) and np.array_equal(hh[:, 1], collected_words(np.arange(65536, dtype=np.uint16).view(np.uint8), YUV422_F16, unit)), "the f16 collection rule at unit %d" % unit
        assert ff.shape == (values.size, 2) and np.array_equal(ff[:, 0], values.view(np.uint32))
        assert np.array_equal(ff[:, 1], collected_words(np.ascontiguousarray(values).view(np.uint8), YUV422_F32, unit)), "the f32 collection rule at unit %d" % unit
        # inversion on the program's own numbers: f32 always, f16 for the 8-bit unit
        back = {int(b): int(w) for b, w in ff}
        assert np.array_equal(collected_words(d[:, 1].astype(np.uint32).view(np.uint8), YUV422_F32, unit), words)
        if unit == 255:
            assert np.unique(d[:, 2]).size == 256 and np.array_equal(hh[d[:, 2], 1], words), "collect(deliver(b)) = b through F16 for all 256 bytes"
        else:
            again = elements(hh[d[:, 2], 1].astype(np.uint16), YUV422_F16, unit).view(np.uint16)
            assert np.array_equal(again, d[:, 2]), "F16 at the 16-bit unit is idempotent"
        del back


# ---- 11. the kernels' times and names (hardware)
def check_kernel_times():
    w, h = SHAPES[0]
    L = lib()
    samples = case_samples("422", w, h)
    q = DQ.Queue(samples[0], "YUY2", FULL, 8)
    try:
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        d = Delivery(q, "YUY2", YUV422_F16, False, 8); d.set()
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        ms, name = L.cfhd_amd_decode_batch_kernel_ms(q.b, 9), L.cfhd_amd_decode_batch_kernel_name(q.b, 9)
        print("k_dec_deliver_yuv422, 8 pictures of %d x %d: %.4f ms" % (w, h, ms))
        assert ms > 0 and name == DELIVER, (ms, name)
        packed = DP.Delivery(q, PACKED, False, 8); packed.set()
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) > 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
    finally:
        q.close()
    frames = geometry_frames("YUY2", w, h, YUV422_F32)
    src = Source(frames, w, h, YUV422_F32, False)
    row = row_bytes("YUY2", w)
    mem = DeviceArray(np.concatenate([collected(f, "YUY2", YUV422_F32).reshape(-1) for f in frames]))
    with Batch(intra("YUY2"), w, h, 4) as bt, Batch(PF.RG48_444, w, h, 4) as rgb:
        assert L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT and L.cfhd_amd_batch_kernel_name(rgb.b, 20) == b"k_enc_collect"
        src.feed(bt.L, bt.b, 0, 2); src.feed(bt.L, bt.b, 2, 2)
        first = bt.run()
        ms = L.cfhd_amd_batch_kernel_ms(bt.b, 20)
        print("k_enc_collect_yuv422, two launches of two frames: %.4f ms" % ms)
        assert ms > 0 and L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT, ms
        for i in range(4): assert L.cfhd_amd_batch_upload_device(bt.b, i, mem.ptr + i * row * h, row) == 0, amd_last_error()
        bt.run()
        assert L.cfhd_amd_batch_kernel_ms(bt.b, 20) == 0, "a pass fed by upload_device has no collect time"
        assert len(set(first)) == 4


# ---- 12. a torch tensor (hardware)
def check_torch(torch):
    """Delivery into a torch tensor (N, 2 * H * W) through its data_ptr(): the two views, Y (N, H, W) and CbCr (N, 2, H, W / 2), against numpy."""
    w, h = SHAPES[0]
    samples = case_samples("422", w, h)
    for fmt, layout, dtype in (("YUY2", YUV422_U8, torch.uint8), ("YUY2", YUV422_F16, torch.float16), ("YU64", YUV422_F32, torch.float32)):
        q = DQ.Queue(samples[0], fmt, FULL, 8)
        try:
            t = torch.zeros((8, 2 * h * w), dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            E = ELEMENT[layout]
            assert lib().cfhd_amd_decode_batch_set_device_pictures(q.b, t.data_ptr(), 2 * h * w * E, w * E, layout) == 0, amd_last_error()
            assert DP.run_pass(q, samples) == (8, [0] * 8)
            want = q.pictures(8)
            Y = t[:, : h * w].view(8, h, w).cpu().numpy()
            C = t[:, h * w:].view(8, 2, h, w // 2).cpu().numpy()
            for i in range(8):
                wy, wc = planes_of(want[i], w, h, fmt, layout)
                assert np.array_equal(np.ascontiguousarray(Y[i]).view(np.uint8).reshape(h, w * E), wy), "%s %s: Y of picture %d" % (fmt, LAYOUT_NAMES[layout], i)
                assert np.array_equal(np.ascontiguousarray(C[i]).view(np.uint8).reshape(2, h, w // 2 * E), wc), "%s %s: CbCr of picture %d" % (fmt, LAYOUT_NAMES[layout], i)
        finally:
            q.close()
