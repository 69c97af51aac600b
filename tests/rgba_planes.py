"""Pictures that carry alpha (b64a, BGRA, BGRa) as planar R, G, B, A tensors in device memory, on both queues: cfhd_amd_decode_batch_set_device_pictures with
CFHD_AMD_PICTURES_RGBA_U8 / _U16 / _F16 / _F32 (k_dec_deliver_rgba: a picture of W x H pixels as four planes R, G, B, A of H rows of W elements at the pitch, the top
row first -- a torch tensor (N, 4, H, W)) and cfhd_amd_batch_upload_device_planar with CFHD_AMD_FRAMES_RGBA_* on every frame batch whose pixel format is one of the
three (k_enc_collect_rgba, the mirror image).  The helpers and test bodies shared by tests/test_gpu_rgba_planes.py (hardware) and tests/test_rgba_planes_emulated.py
(the same functions inside cfhd_testlib.emulated_product(), where a device pointer is a host pointer).

Every comparison is exact; the float layouts are compared as bit patterns.  The witnesses are independent of the two kernels: a delivered picture is held to
cfhd_amd_decode_batch_download_output of the same pass, de-interleaved by numpy and flipped for BGRA (split) -- the 8-bit outputs dither with a seed that follows the
pass, so the handle is no witness for them; one b64a case is held to ONE CFHD_DecodeSample handle as well --; collected frames to cfhd_amd_batch_download_frame;
samples to those of a batch of the same kind fed the numpy-interleaved frames (pack) through cfhd_amd_batch_upload.  The element rules in numpy are those of
tests/yuv422_planes.py (elements, collected_words), with the unit of the format's own word: 255 for BGRA / BGRa, 65535 for b64a.  Alpha is a component like the
others.  Device buffers are checked whole: filled with a pattern, guards in front and behind, and afterwards equal to the pattern with exactly the row bytes of the
planes replaced (deliveries) or byte for byte what they were (sources).
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import group_decode_queue as GQ
import device_pictures as DP
import planar_frames as PF
import yuv422_planes as YP
import gop_input_frames
from device_pictures import DeviceArray, pattern, GUARD
from decode_queue import use_emulated, V, FULL, HALF
from yuv422_planes import compare_frame, chunked

PACKED = 0
RGBA_U8, RGBA_U16, RGBA_F16, RGBA_F32 = 11, 12, 13, 14
LAYOUT_NAMES = {RGBA_U8: "u8", RGBA_U16: "u16", RGBA_F16: "f16", RGBA_F32: "f32"}
ELEMENT = {RGBA_U8: 1, RGBA_U16: 2, RGBA_F16: 2, RGBA_F32: 4}
FORMATS = ["b64a", "BGRA", "BGRa"]
PIX = {"b64a": PIX_B64A, "BGRA": PIX_BGRA, "BGRa": PIX_BGRa}
UNIT = {"b64a": 65535, "BGRA": 255, "BGRa": 255}
# the positions of R, G, B, A among the four words (bytes) of a pixel; BGRA has the bottom row first in its packed form
ORDER = {"b64a": (1, 2, 3, 0), "BGRA": (2, 1, 0, 3), "BGRa": (2, 1, 0, 3)}
BOTTOM_UP = {"b64a": False, "BGRA": True, "BGRa": False}
SHAPE = (192, 96)
DELIVER, COLLECT = b"k_dec_deliver_rgba", b"k_enc_collect_rgba"
FILMSCAN2 = PF.FILMSCAN2
# the texts the batches outside the family have for the values 11 .. 14, and the batches of the family for the values below 11: recorded from the library as it was
# before these layouts existed
PARENT_DECODE_UNKNOWN = "decode queue: unknown layout of the device pictures"
PARENT_DECODE_PLANAR = "decode queue: the planar layouts serve batches whose output is RG48"
PARENT_DECODE_YUV422 = "decode queue: the 4:2:2 plane layouts serve batches whose output is YUY2, 2vuy or YU64"
PARENT_FRAMES_NOT_RG48 = "frames from planar tensors: the batch's input is not RG48"
PARENT_FRAMES_NOT_BYR4 = "frames from planar tensors: the batch's input is not BYR4"
PARENT_FRAMES_UNKNOWN = "frames from planar tensors: unknown layout"
PARENT_FRAMES_BYR4 = "frames from planar tensors: a BYR4 batch takes the four planes of a mosaic (the BAYER layouts) and no other layout"
PARENT_FRAMES_YUV422 = "frames from planar tensors: the 4:2:2 plane layouts serve batches whose input is YUY2, 2vuy or YU64"


def lib(): return YP.lib()
def word(fmt): return np.uint16 if fmt == "b64a" else np.uint8
def native(fmt): return RGBA_U16 if fmt == "b64a" else RGBA_U8
def layouts_of(fmt): return [native(fmt), RGBA_F16, RGBA_F32]
def row_bytes(fmt, w): return w * 4 * np.dtype(word(fmt)).itemsize
def as_yuv422(layout): return layout - RGBA_U8 + YP.YUV422_U8      # (the element types of the two families are the same four; the numpy rules are written once)


# ---- the two views of a picture, and the element rules
def split(picture, w, h, fmt):
    """A packed picture -> the planes R, G, B, A, top row first, [4, h, w] in the format's own word."""
    px = np.ascontiguousarray(picture).reshape(-1).view(word(fmt)).reshape(h, w, 4)
    if BOTTOM_UP[fmt]: px = px[::-1]
    return np.ascontiguousarray(px[:, :, list(ORDER[fmt])].transpose(2, 0, 1))


def pack(planes, fmt):
    """Planes [4, h, w] in the format's word -> the packed frame, uint8 [h, row bytes]."""
    _, h, w = planes.shape
    px = np.empty((h, w, 4), word(fmt))
    for c, k in enumerate(ORDER[fmt]): px[:, :, k] = planes[c]
    if BOTTOM_UP[fmt]: px = px[::-1]
    return np.ascontiguousarray(px).reshape(h, 4 * w).view(np.uint8)


def elements(words, layout, unit): return YP.elements(words, as_yuv422(layout), unit)
def collected_words(bytes_, layout, unit): return YP.collected_words(bytes_, as_yuv422(layout), unit)


def planes_of(picture, w, h, fmt, layout):
    """The planes of a packed picture in the element type of `layout` by the delivery rule: uint8 [4, h, w * E]."""
    return elements(split(picture, w, h, fmt), layout, UNIT[fmt])


def collected(planes, fmt, layout):
    """Planes of elements (uint8 [4, h, w * E]) -> the packed frame the collection rule gives, uint8 [h, row bytes]."""
    return pack(collected_words(planes, layout, UNIT[fmt]), fmt)


def geometry(w, h, layout, padded):
    """(plane row bytes, pitch, stride): the pitch the row bytes rounded up to 16 -- where they are a multiple of 16 the contiguous tensor (n, 4, H, W) --, or that + 48
    and a stride of + 4096."""
    row = w * ELEMENT[layout]
    pitch = ((row + 15) & ~15) + (48 if padded else 0)
    return row, pitch, 4 * h * pitch + (4096 if padded else 0)


def place(image, at, pitch, h, row, planes):
    image[at: at + 4 * h * pitch].reshape(4 * h, pitch)[:, :row] = np.asarray(planes).reshape(4 * h, row)


class Delivery(DP.Delivery):
    """device_pictures.Delivery for the four planes of the pictures of a decode batch whose output is b64a, BGRA or BGRa."""
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
    """planar_frames.Source for frames of four planes (uint8 [4, h, w * E]) of w x h pictures."""
    def __init__(self, frames, w, h, layout, padded):
        self.w, self.h, self.layout, self.n = w, h, layout, len(frames)
        self.row, self.pitch, self.stride = geometry(w, h, layout, padded)
        self.image = pattern(GUARD + self.n * self.stride + GUARD)
        for i, f in enumerate(frames): place(self.image, GUARD + i * self.stride, self.pitch, h, self.row, f)
        self.mem = DeviceArray(self.image)


Batch = PF.Batch
ENCODED = {"4444": ENCODED_RGBA4444, "444": ENCODED_RGB444, "422": ENCODED_YUV422}


def intra(fmt, encoded): return ("ex", PIX[fmt], ENCODED[encoded], 0, QUALITY_FILMSCAN1)


def frame_planes(fmt, w, h, n=4):
    """n textured frames of the format, all different, alpha a component of its own: the planes [4, h, w] in the format's word."""
    frames, pitch = gop_input_frames.frames(fmt, w, h, n)
    assert pitch == row_bytes(fmt, w)
    return [split(f, w, h, fmt) for f in frames]


# ---- 1. delivery equals numpy on download_output of the same pass
# name: (kind of sample, output, w, h of the sample, resolution, layouts, what it exercises)
DECODE_CASES = {
    "1-rgba-b64a": ("4444", "b64a", 192, 96, FULL, (RGBA_U16, RGBA_F16, RGBA_F32)),             # 24 lanes, a partial wave; real alpha; held to the handle too
    "2-rgba-b64a-half-100x32": ("4444", "b64a", 200, 64, HALF, (RGBA_U16, RGBA_F32)),           # the 4-column tail behind 12 whole groups
    "3-rgb444-b64a-528x64": ("444", "b64a", 528, 64, FULL, (RGBA_U16, RGBA_F16)),               # 66 lanes, a row crosses the wave; constant alpha
    "4-422-b64a-208x104": ("422", "b64a", 208, 104, FULL, (RGBA_U16, RGBA_F32)),
    "5-rgba-bgra": ("4444", "BGRA", 192, 96, FULL, (RGBA_U8, RGBA_F16, RGBA_F32)),              # bottom row first; real alpha
    "6-rgb444-bgra-200x64": ("444", "BGRA", 200, 64, FULL, (RGBA_U8, RGBA_F16)),                # width % 16 = 8: the tail
    "7-422-bgra_top-320x240": ("422", "BGRa", 320, 240, FULL, (RGBA_U8, RGBA_F32)),             # dithered, top row first
    "8-422-bgra_top-1040x40": ("422", "BGRa", 1040, 40, FULL, (RGBA_U8, RGBA_F16)),             # 65 groups of 16: a lane's second trip
    "9-groups-b64a-320x240": ("groups", "b64a", 320, 240, FULL, (RGBA_U16, RGBA_F16)),
}
DECODE_IDS = list(DECODE_CASES)
_handle = {}


def case_samples(kind, w, h):
    if kind == "groups": return GQ.group_stream("amd", w, h, 0)
    return DQ.samples_of(kind, w, h, DP.source() if (w, h) == SHAPE else "amd")


def check_delivery(name):
    """Every layout of the case, into the tight geometry and into a pitch of + 48 with a stride of + 4096 (filled with a canary that must survive), on one batch: the
    layout is switched between passes."""
    kind, fmt, w, h, resolution, layouts = DECODE_CASES[name]
    samples = case_samples(kind, w, h)
    q = YP.case_queue(kind, samples, fmt, resolution)
    L = lib()
    try:
        assert (q.w, q.h) == ((w, h) if resolution == FULL else (w // 2, h // 2)) and q.row_bytes == row_bytes(fmt, q.w)
        if name.startswith("2-"): assert q.w == 100 and q.w // 8 == 12 and q.w % 8 == 4
        if name.startswith("3-"): assert q.w // 8 == 66
        if name.startswith("6-"): assert q.w % 16 == 8
        if name.startswith("8-"): assert q.w // 16 == 65
        handle = None
        if name.startswith("1-"):                               # b64a carries no dither: the handle's pictures are the pass's
            res, geo = DQ.handle_pictures(samples, fmt, resolution)
            assert [rc for rc, _ in res] == [0] * 8 and geo == (q.w, q.h, q.row_bytes)
            handle = [p for _, p in res]
        for layout in layouts:
            for padded in (False, True):
                what = "%s, %s, %s" % (name, LAYOUT_NAMES[layout], "pitch + 48, stride + 4096" if padded else "the smallest pitch")
                d = Delivery(q, fmt, layout, padded, 8)
                if not padded and d.row % 16 == 0: assert d.pitch == q.w * ELEMENT[layout] and d.stride == 4 * q.h * d.pitch      # a contiguous (8, 4, H, W) tensor
                if padded: assert d.pitch == ((d.row + 15) & ~15) + 48 and d.stride == 4 * q.h * d.pitch + 4096
                d.set()
                assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
                ret, status = DP.run_pass(q, samples)
                assert ret == 8 and status == [0] * 8, (what, ret, status, amd_last_error())
                want = q.pictures(8)
                assert len(set(p.tobytes() for p in want)) == 8
                alpha = np.unique(np.concatenate([split(p, q.w, q.h, fmt)[3].reshape(-1) for p in want]))
                if kind == "4444": assert alpha.size > 100, "%s: the alpha of an RGBA sample takes only %d values" % (name, alpha.size)
                elif fmt == "b64a": assert list(alpha) == [0xfff0 if kind == "444" else 0xffff], "%s: the constant alpha is %s" % (name, alpha)
                else: assert alpha.size == 1
                if handle is not None:
                    for i in range(8): assert np.array_equal(want[i], handle[i]), "%s: download_output(%d) differs from the handle's picture" % (what, i)
                d.check(want, what)
    finally:
        q.close()


# ---- 2. a short pass touches nothing else; switching to PACKED, to NULL and back, the name under index 9 each time
def check_short_pass_and_switching(fmt, layout):
    w, h = SHAPE
    samples = case_samples("4444", w, h)
    q = DQ.Queue(samples[0], fmt, FULL, 8)
    L = lib()
    try:
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        d = Delivery(q, fmt, layout, True, 8)
        assert d.pitch > d.row and d.stride > 4 * h * d.pitch
        d.set()
        ret, status = DP.run_pass(q, samples, count=3)
        assert (ret, status) == (3, [0] * 3)
        d.check(q.pictures(3) + [None] * 5, "count = 3 of 8: planes, padding, gaps, the pictures behind the count, the guards")
        packed = DP.Delivery(q, PACKED, True, 8); packed.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        ret, status = DP.run_pass(q, samples[5:8])
        assert (ret, status) == (3, [0] * 3)
        packed.check(q.pictures(3) + [None] * 5, "PACKED behind an RGBA layout")
        d.check([None] * 8, "the planes while PACKED is set")
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check([None] * 8, "the planes after set_device_pictures(NULL)"); packed.check([None] * 8, "the packed buffer after set_device_pictures(NULL)")
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        other = [l for l in layouts_of(fmt) if l != layout][0]
        d2 = Delivery(q, fmt, other, False, 8); d2.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d2.check(q.pictures(8), "%s behind NULL" % LAYOUT_NAMES[other])
        d.check([None] * 8, "the first buffer while another is set")
        d.set()
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check(q.pictures(8), "count = 8 behind PACKED, NULL and %s" % LAYOUT_NAMES[other])
    finally:
        q.close()


# ---- 3. verdicts and the slow path
def check_verdicts(fmt, layout):
    """device_pictures.check_verdicts' pass -- a damaged code stream (every sample the parser passed goes through the handle inside wait and is delivered by the second
    launch there), a size that is no multiple of 4 (the slow path's), a sample the parser refuses for good --: zeros (0.0) in all four planes where a sample failed,
    the picture download_output gives everywhere else, the status as wait gives it: the handle's."""
    w, h = SHAPE
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
            if fmt == "b64a": assert np.array_equal(got[i], res[i][1]), "picture %d differs from the handle's" % i
        d.check(got, "verdicts, %s %s" % (fmt, LAYOUT_NAMES[layout]))
        failed = codes.index(next(rc for rc in codes if rc))
        at = GUARD + failed * d.stride
        assert not d.mem.read()[at: at + 4 * h * d.pitch].reshape(4 * h, d.pitch)[:, : d.row].any(), "the four planes of a failed sample are 0 (0.0)"
        ret, status = DP.run_pass(q, intact)
        assert ret == 8 and status == [0] * 8
        d.check(q.pictures(8), "an intact pass behind the damaged one")
    finally:
        q.close()


# ---- 4. collection equals numpy: the rules
RULE_W, RULE_H, RULE_N = 192, 96, 2
RULE_ELEMENTS = RULE_N * 4 * RULE_W * RULE_H                       # 147 456


def f32_rule_values(unit):
    """yuv422_planes.f32_rule_values of the unit -- the exact ties of x * unit and their neighbours, 0.5, zeros, infinities, NaNs, negatives, 1 and beyond, the smallest
    subnormal, random patterns -- and random 32-bit patterns of its own for the rest of the two frames."""
    first = YP.f32_rule_values(unit)
    rest = np.random.default_rng(23).integers(0, 1 << 32, RULE_ELEMENTS - first.size, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([first, rest])


def rule_frames(fmt, layout):
    """Two frames of planes (147 456 elements).  U8: every byte; U16 and F16: i * 40503 mod 65536 over consecutive i -- every word, every binary16 pattern, its
    subnormals, infinities and NaNs among them; F32: f32_rule_values of the format's unit."""
    if layout == RGBA_U8: flat = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 37 + 11) & 0xff).astype(np.uint8)
    elif layout in (RGBA_U16, RGBA_F16):
        flat = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 40503) & 0xffff).astype(np.uint16)
        assert np.unique(flat).size == 65536
    else: flat = f32_rule_values(UNIT[fmt])
    return list(np.ascontiguousarray(flat).view(np.uint8).reshape(RULE_N, 4, RULE_H, RULE_W * ELEMENT[layout]))


def check_collection(fmt, layout):
    w, h, n = RULE_W, RULE_H, RULE_N
    unit = UNIT[fmt]
    frames = rule_frames(fmt, layout)
    # what the rule says of the named values, whatever the frames hold
    one = lambda x, l: int(collected_words(np.array([x], np.float32 if l == RGBA_F32 else np.float16).view(np.uint8), l, unit)[0])
    for l in (RGBA_F16, RGBA_F32):
        assert one(0.5, l) == (128 if unit == 255 else 32768), "0.5: an exact tie, to even"
        assert one(np.nan, l) == 0 and one(-np.inf, l) == 0 and one(np.inf, l) == unit and one(-0.0, l) == 0 and one(-0.25, l) == 0 and one(1.0, l) == unit and one(2.0, l) == unit
    sub = collected_words(np.array([0x03ff, 0x0001], np.uint16).view(np.uint8), RGBA_F16, unit)      # binary16 subnormals: 1023 x 2^-24 and 2^-24
    assert list(sub) == ([0, 0] if unit == 255 else [4, 0])
    with Batch(intra(fmt, "4444"), w, h, n) as bt:
        src = Source(frames, w, h, layout, False)
        assert src.pitch == w * ELEMENT[layout] and src.stride == 4 * h * src.pitch      # a contiguous (2, 4, H, W) tensor
        src.feed(bt.L, bt.b, 0, n)
        for i in range(n): compare_frame(bt.frame(i, row_bytes(fmt, w)), collected(frames[i], fmt, layout), "%s %s, frame %d" % (fmt, LAYOUT_NAMES[layout], i))
        src.unchanged("%s %s" % (fmt, LAYOUT_NAMES[layout]))


# ---- 5. inversion
def all_words_pictures(fmt):
    """Two 192 x 96 pictures (147 456 components): BGRA / BGRa, every byte in each of the four components of each picture; b64a, every one of the 65 536 words, a
    quarter of them in each component."""
    if fmt == "b64a": words = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 40503 + 977) & 0xffff).astype(np.uint16)
    else: words = np.random.default_rng(5).integers(0, 256, RULE_ELEMENTS).astype(np.uint8)
    pictures = list(words.view(np.uint8).reshape(RULE_N, RULE_H, row_bytes(fmt, RULE_W)))
    for p in pictures:
        planes = split(p, RULE_W, RULE_H, fmt)
        if fmt != "b64a": assert all(np.unique(planes[c]).size == 256 for c in range(4))
    assert np.unique(words).size == UNIT[fmt] + 1
    return pictures


def check_inversion(fmt, layout):
    """collect(deliver(w)) = w: for the 8-bit unit through U8, F32 and F16 alike, for the 16-bit unit through U16 and F32; through F16 at the 16-bit unit, delivering
    what was collected returns every delivered bit pattern."""
    w, h, n = RULE_W, RULE_H, RULE_N
    pictures = all_words_pictures(fmt)
    planes = [planes_of(p, w, h, fmt, layout) for p in pictures]
    exact = not (fmt == "b64a" and layout == RGBA_F16)
    with Batch(intra(fmt, "4444"), w, h, n) as bt:
        src = Source(planes, w, h, layout, False)
        src.feed(bt.L, bt.b, 0, n)
        for i in range(n):
            got = bt.frame(i, row_bytes(fmt, w))
            if exact: compare_frame(got, pictures[i], "%s %s of the delivered picture %d" % (fmt, LAYOUT_NAMES[layout], i))
            else: assert np.array_equal(planes_of(got, w, h, fmt, layout), planes[i]), "f16: picture %d delivered, collected and delivered again" % i


# ---- 6. every kind of frame batch: the frame in the slot equals numpy's, the samples equal those of a batch fed the packed frames through cfhd_amd_batch_upload
# name: (format, kind, w, h, mode, CFHD_AMD_CHUNK, layouts, runs: (first, count) in call order)
WHOLE = ((0, 4),)
KINDS = {
    "10-b64a-rgba4444": ("b64a", intra("b64a", "4444"), 192, 96, 1, None, (RGBA_U16, RGBA_F16, RGBA_F32), WHOLE),
    "11-b64a-rgb444": ("b64a", intra("b64a", "444"), 208, 104, 1, None, (RGBA_F16,), WHOLE),      # the A plane is read, the encoder drops it
    "12-b64a-422": ("b64a", intra("b64a", "422"), 208, 104, 1, None, (RGBA_U16,), WHOLE),
    "13-bgra-rgba4444": ("BGRA", intra("BGRA", "4444"), 192, 96, 1, None, (RGBA_U8, RGBA_F16, RGBA_F32), WHOLE),      # bottom row first
    "14-bgra_top-422": ("BGRa", intra("BGRa", "422"), 320, 240, 1, None, (RGBA_U8, RGBA_F32), WHOLE),
    "15-bgra-groups": ("BGRA", ("groups", PIX_BGRA, 0, 0, QUALITY_FILMSCAN1), 320, 240, 1, None, (RGBA_U8,), WHOLE),
    "15-bgra-groups-middle": ("BGRA", ("groups", PIX_BGRA, 0, 0, QUALITY_FILMSCAN1), 320, 240, 1, None, (RGBA_F16,), ((1, 2),)),
    "group-stream-b64a": ("b64a", ("group_stream", PIX_B64A, 0, 0, QUALITY_FILMSCAN1), 192, 96, 1, None, (RGBA_U16,), WHOLE),
    "17-bgra_top-chunks": ("BGRa", intra("BGRa", "422"), 192, 96, 1, "3", (RGBA_U8,), ((1, 3), (0, 1))),      # frames 0 - 2 | 3: the first run crosses the cut
}
KIND_IDS = list(KINDS)


def check_kind(name):
    fmt, kind, w, h, mode, chunk, layouts, runs = KINDS[name]
    row = row_bytes(fmt, w)
    words = frame_planes(fmt, w, h)
    for layout in layouts:
        src = Source([elements(p, layout, UNIT[fmt]) for p in words], w, h, layout, True)
        frames = [collected(f, fmt, layout) for f in (elements(p, layout, UNIT[fmt]) for p in words)]
        if layout != RGBA_F16 or fmt != "b64a":
            for i in range(4): compare_frame(frames[i], pack(words[i], fmt), "%s: numpy's own inversion, frame %d" % (name, i))
        assert len(set(f.tobytes() for f in frames)) == 4
        held = [np.ascontiguousarray(frames[(i + 2) % 4][::-1]) for i in range(4)]      # what the slots hold before the runs
        fed = set(i for first, count in runs for i in range(first, first + count))
        in_slots = [frames[i] if i in fed else held[i] for i in range(4)]
        with chunked(chunk), Batch(kind, w, h, 4, mode) as twin:
            twin.upload(in_slots, row)
            first = twin.run()
        with chunked(chunk), Batch(kind, w, h, 4, mode) as bt:
            assert bt.L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT
            bt.upload(held, row)
            for at, count in runs: src.feed(bt.L, bt.b, at, count)
            for i in range(4): compare_frame(bt.frame(i, row), in_slots[i], "%s, %s: frame %d in front of the pass" % (name, LAYOUT_NAMES[layout], i))
            second = bt.run()
            for i in range(4): assert second[i] == first[i], "%s, %s: sample %d of the batch fed from planes differs (%d / %d bytes)" % (name, LAYOUT_NAMES[layout], i, len(second[i]), len(first[i]))
            for i in range(4): compare_frame(bt.frame(i, row), in_slots[i], "%s: frame %d behind the pass" % (name, i))
        src.unchanged(name)


def check_stream(fmt="BGRa", layout=RGBA_U8):
    """cfhd_amd_batch_create_stream with rate feedback (tables that move), two passes: the samples of both passes equal those of a stream fed the packed frames."""
    w, h = SHAPE
    kind = ("stream", PIX[fmt], ENCODED_YUV422, 0, FILMSCAN2)
    row = row_bytes(fmt, w)
    words = frame_planes(fmt, w, h, 8)
    packed = [pack(p, fmt) for p in words]
    assert lib().cfhd_amd_quantizer_is_static(w, h, PIX[fmt], ENCODED_YUV422, 0, FILMSCAN2) == 0, "the tables of this stream move"
    with Batch(kind, w, h, 4) as twin:
        twin.upload(packed[:4], row); first = [twin.run()]
        twin.upload(packed[4:], row); first.append(twin.run())
    src = Source([elements(p, layout, UNIT[fmt]) for p in words], w, h, layout, True)
    with Batch(kind, w, h, 4) as bt:
        assert bt.L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT
        for k in range(2):
            src.feed(bt.L, bt.b, 0, 4, src_first=4 * k)
            for i in range(4): compare_frame(bt.frame(i, row), packed[4 * k + i], "stream, pass %d: frame %d" % (k, i))
            second = bt.run()
            for i in range(4): assert second[i] == first[k][i], "stream, pass %d: sample %d of the stream fed from planes differs" % (k, i)
        assert first[0] != first[1]
    src.unchanged("stream")


# ---- 7. the chain, all in HBM: decode queue -> planes -> frame queue
def check_chain(fmt, layout):
    """Decode batch -> planes -> frame batch: cfhd_amd_batch_download_frame equals the decode's packed picture (download_output of the same pass) -- deliver, then
    collect, on the device; for F16 at the 16-bit unit the picture delivered again equals the planes."""
    w, h = SHAPE
    samples = case_samples("4444", w, h)
    row = row_bytes(fmt, w)
    q = DQ.Queue(samples[0], fmt, FULL, 8)
    try:
        d = Delivery(q, fmt, layout, True, 8); d.set()
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        pictures = q.pictures(8)
        with Batch(intra(fmt, "4444"), w, h, 8) as bt:
            assert bt.L.cfhd_amd_batch_upload_device_planar(bt.b, 0, 8, d.mem.ptr + GUARD, d.stride, d.pitch, layout) == 0, amd_last_error()
            for i in range(8):
                got = bt.frame(i, row)
                if fmt == "b64a" and layout == RGBA_F16: assert np.array_equal(planes_of(got, w, h, fmt, layout), planes_of(pictures[i], w, h, fmt, layout)), "f16: frame %d of the chain, delivered again" % i
                else: compare_frame(got, pictures[i].reshape(h, row), "%s %s: frame %d of the chain" % (fmt, LAYOUT_NAMES[layout], i))
            assert len(set(bt.run())) == 8
        d.check(pictures, "the delivered planes behind the frame queue's pass")
    finally:
        q.close()


# ---- 8. gates
def check_decode_gates():
    w, h = SHAPE
    L = lib()
    yuv = case_samples("422", w, h)
    import bayer_queue as BQ
    queues = {name: DQ.Queue(yuv[0], name, FULL, 8 if name in ("b64a", "BGRA") else 2) for name in ("b64a", "BGRA", "BGRa", "YU64", "v210", "RG48")}
    bayer = BQ.Queue(BQ.samples_of(w, h, "amd")[0], 2)
    try:
        q, q8 = queues["b64a"], queues["BGRA"]
        d = Delivery(q, "b64a", RGBA_F32, True, 8)
        p, stride, pitch = d.mem.ptr + GUARD, d.stride, d.pitch
        def refused(queue, ptr, s, pt, layout, what):
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, ptr, s, pt, layout) == -1, what
            text = amd_last_error()
            assert text and "decode queue" in text, "%s: refused without a text (%r)" % (what, text)
            return text
        # the layouts are served where they belong
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, p, stride, pitch, RGBA_F32) == 0, amd_last_error()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER and L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        # what must not move: 11 .. 14 on every batch outside the family; 1 .. 10 and -1 on a b64a and a BGRA batch (0, PACKED, is served there)
        for name in ("YU64", "v210", "RG48"):
            for layout in (11, 12, 13, 14): assert refused(queues[name], p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_DECODE_UNKNOWN
        for layout in (11, 12, 13, 14): assert refused(bayer, p, stride, pitch, layout, "layout %d on a Bayer batch" % layout) == PARENT_DECODE_UNKNOWN
        for name in ("b64a", "BGRA"):
            for layout in (1, 2, 3): assert refused(queues[name], p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_DECODE_PLANAR
            for layout in (4, 5, 6, -1, 15): assert refused(queues[name], p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_DECODE_UNKNOWN
            for layout in (7, 8, 9, 10): assert refused(queues[name], p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_DECODE_YUV422
            assert L.cfhd_amd_decode_batch_set_device_pictures(queues[name].b, p, stride, queues[name].row_bytes, PACKED) == 0, amd_last_error()
            assert L.cfhd_amd_decode_batch_set_device_pictures(queues[name].b, None, 0, 0, 0) == 0
        parent = {PARENT_DECODE_UNKNOWN, PARENT_DECODE_PLANAR, PARENT_DECODE_YUV422}
        # the new refusals
        u8 = refused(q, p, stride, pitch, RGBA_U8, "U8 on a b64a batch")
        u16 = set(refused(queues[name], p, stride, pitch, RGBA_U16, "U16 on a %s batch" % name) for name in ("BGRA", "BGRa"))
        low_pitch = set(refused(q, p, stride, w * ELEMENT[layout] - 16, layout, "a pitch below W x element size, %s" % LAYOUT_NAMES[layout]) for layout in layouts_of("b64a"))
        low_pitch |= set(refused(q8, p, stride, w * ELEMENT[layout] - 16, layout, "a pitch below W x element size, BGRA %s" % LAYOUT_NAMES[layout]) for layout in layouts_of("BGRA"))
        low_pitch.add(refused(q, p, stride, -pitch, RGBA_F32, "a negative pitch"))
        smallest = lambda pt, layout: pt * (4 * h - 1) + w * ELEMENT[layout]
        low_stride = set(refused(q, p, smallest(pt, layout) - 16, pt, layout, "a stride below the four planes, %s" % LAYOUT_NAMES[layout]) for layout, pt in ((RGBA_U16, pitch), (RGBA_F16, w * 2), (RGBA_F32, pitch)))
        low_stride.add(refused(q8, p, smallest(w, RGBA_U8) - 16, w, RGBA_U8, "a stride below the four planes, BGRA u8"))
        off = set([refused(q, p + 8, stride, pitch, RGBA_F32, "a pointer off 16"), refused(q, p, stride + 8, pitch, RGBA_F32, "a stride off 16"), refused(q, p, stride, pitch + 8, RGBA_F32, "a pitch off 16")])
        for s in (u16, low_pitch, low_stride, off): assert len(s) == 1, s
        new = {u8} | u16 | low_pitch | low_stride
        assert len(new) == 4 and not (new & parent) and not (new & off), "the texts of the new refusals are distinct from each other and from the existing ones"
        existing = set([refused(queues["YU64"], p, stride, queues["YU64"].row_bytes - 16, PACKED, "a low pitch, packed"), refused(queues["YU64"], p, 16, pitch, PACKED, "a low stride, packed"),
                        refused(queues["YU64"], p, stride, 64, YP.YUV422_U16, "a low pitch, 4:2:2 planes"), refused(queues["YU64"], p, 32, pitch - pitch % 32, YP.YUV422_U16, "a low stride, 4:2:2 planes"),
                        refused(queues["YU64"], p, stride, pitch, YP.YUV422_U8, "YUV422_U8 on a YU64 batch")])
        assert not (new & existing), (new, existing)
        # the smallest pitch and stride are served
        for layout in layouts_of("b64a"):
            row = w * ELEMENT[layout]
            assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, p, smallest(row, layout), row, layout) == 0, amd_last_error()
        assert L.cfhd_amd_decode_batch_set_device_pictures(q8.b, p, smallest(w, RGBA_U8), w, RGBA_U8) == 0, amd_last_error()
        assert L.cfhd_amd_decode_batch_set_device_pictures(q8.b, None, 0, 0, 0) == 0
        # a refusal leaves the layout that was set in place, and nothing was launched: the memory holds what was there
        refused(q, p, stride, w * 4 - 16, RGBA_F32, "a pitch below the row bytes, again")
        d.check([None] * 8, "behind refused calls")
        # a pass in flight refuses
        d.set()
        blob, offsets, sizes = DQ.pack(yuv)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        try:
            assert "flight" in refused(q, p, stride, pitch, RGBA_F32, "a pass in flight")
        finally:
            ret, status = q.wait(8)
        assert ret == 8 and status == [0] * 8
        d.check(q.pictures(8), "the pass the refused calls were made in")
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER and L.cfhd_amd_decode_batch_kernel_name(queues["RG48"].b, 9) == b"k_dec_deliver"
    finally:
        for x in queues.values(): x.close()
        bayer.close()


def check_frame_gates():
    w, h = SHAPE
    L = lib()
    import bayer_planes as BP
    words = frame_planes("b64a", w, h)
    frames = [elements(p, RGBA_F32, 65535) for p in words]
    src = Source(frames, w, h, RGBA_F32, True)
    p, stride, pitch = src.at(0), src.stride, src.pitch
    row = row_bytes("b64a", w)
    def refused(b, first, count, ptr, s, pt, layout, what):
        assert L.cfhd_amd_batch_upload_device_planar(b, first, count, ptr, s, pt, layout) == -1, what
        text = amd_last_error()
        assert text and "planar" in text, "%s: refused without a text (%r)" % (what, text)
        return text
    # the layouts are served where they belong
    with Batch(intra("b64a", "422"), w, h, 4) as served:
        src.feed(served.L, served.b, 0, 4)
        for i in range(4): compare_frame(served.frame(i, row), collected(frames[i], "b64a", RGBA_F32), "a b64a batch that encodes to 4:2:2, frame %d" % i)
    # what must not move: 11 .. 14 on the batches outside the family
    with BP.Batch(BP.EX, w, h, 4) as byr4:
        for layout in (11, 12, 13, 14): assert refused(byr4.b, 0, 1, p, stride, pitch, layout, "layout %d on a BYR4 batch" % layout) == PARENT_FRAMES_BYR4
    with Batch(PF.RG48_444, w, h, 4) as rg48:
        for layout in (11, 12, 13, 14): assert refused(rg48.b, 0, 1, p, stride, pitch, layout, "layout %d on an RG48 batch" % layout) == PARENT_FRAMES_UNKNOWN
    for name, pix in (("YUY2", PIX_YUY2), ("v210", PIX_V210)):
        with Batch(("ex", pix, ENCODED_YUV422, 0, QUALITY_FILMSCAN1), w, h, 4) as other:
            for layout in (11, 12, 13, 14): assert refused(other.b, 0, 1, p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_FRAMES_NOT_RG48
    # ... and 0 .. 10, -1 and 15 on a b64a and a BGRA batch
    parent = {PARENT_FRAMES_NOT_RG48, PARENT_FRAMES_NOT_BYR4, PARENT_FRAMES_YUV422, PARENT_FRAMES_UNKNOWN, PARENT_FRAMES_BYR4}
    with Batch(intra("BGRA", "4444"), w, h, 4) as bgra, Batch(intra("b64a", "4444"), w, h, 4) as bt:
        for name, x in (("BGRA", bgra), ("b64a", bt)):
            for layout in (0, 1, 2, 3, -1, 15): assert refused(x.b, 0, 1, p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_FRAMES_NOT_RG48
            for layout in (4, 5, 6): assert refused(x.b, 0, 1, p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_FRAMES_NOT_BYR4
            for layout in (7, 8, 9, 10): assert refused(x.b, 0, 1, p, stride, pitch, layout, "layout %d on a %s batch" % (layout, name)) == PARENT_FRAMES_YUV422
        b = bt.b
        # the new refusals
        t_u8 = refused(b, 0, 1, p, stride, pitch, RGBA_U8, "U8 on a b64a batch")
        t_u16 = refused(bgra.b, 0, 1, p, stride, pitch, RGBA_U16, "U16 on a BGRA batch")
        t_low = set(refused(b, 0, 1, p, stride, w * ELEMENT[layout] - 16, layout, "a pitch below W x element size, %s" % LAYOUT_NAMES[layout]) for layout in layouts_of("b64a"))
        t_low.add(refused(b, 0, 1, p, stride, -pitch, RGBA_F32, "a negative pitch")); t_low.add(refused(bgra.b, 0, 1, p, stride, w - 16, RGBA_U8, "a pitch below W, BGRA u8"))
        t_stride = set(refused(b, 0, 2, p, 4 * h * pt - 16, pt, layout, "a stride below the four planes, %s" % LAYOUT_NAMES[layout]) for layout, pt in ((RGBA_U16, pitch), (RGBA_F16, w * 2), (RGBA_F32, pitch)))
        t_stride.add(refused(bgra.b, 0, 2, p, 4 * h * w - 16, w, RGBA_U8, "a stride below the four planes, BGRA u8"))
        t_off = set([refused(b, 0, 1, p + 8, stride, pitch, RGBA_F32, "a pointer off 16"), refused(b, 0, 2, p, stride + 8, pitch, RGBA_F32, "a stride off 16"), refused(b, 0, 1, p, stride, pitch + 8, RGBA_F32, "a pitch off 16")])
        t_run = set([refused(b, 0, 0, p, stride, pitch, RGBA_F32, "count 0"), refused(b, 3, 2, p, stride, pitch, RGBA_F32, "a run that leaves the batch"), refused(b, -1, 1, p, stride, pitch, RGBA_F32, "a run in front of the batch")])
        t_null = refused(b, 0, 1, None, stride, pitch, RGBA_F32, "no pointer")
        for s in (t_low, t_stride, t_off, t_run): assert len(s) == 1, s
        new = {t_u8, t_u16} | t_low | t_stride
        assert len(new) == 4 and not (new & parent) and not (new & (t_off | t_run | {t_null})), "the texts of the new refusals are distinct from each other and from the existing ones"
        with Batch(YP.intra("YU64"), w, h, 4) as yu64:
            existing = set([refused(yu64.b, 0, 1, p, stride, 64, YP.YUV422_U16, "a low pitch, 4:2:2 planes"), refused(yu64.b, 0, 2, p, 64, pitch - pitch % 32, YP.YUV422_U16, "a low stride, 4:2:2 planes"),
                            refused(yu64.b, 0, 1, p, stride, pitch, YP.YUV422_U8, "YUV422_U8 on a YU64 batch")])
        with Batch(PF.RG48_444, w, h, 4) as rg48:
            existing |= set([refused(rg48.b, 0, 1, p, stride, 64, 1, "a low pitch, RG48 planes"), refused(rg48.b, 0, 2, p, 64, pitch, 1, "a low stride, RG48 planes")])
        assert not (new & existing), (new, existing)
        # nothing was launched: the frames are what upload put there
        held = [np.ascontiguousarray(collected(f, "b64a", RGBA_F32)[::-1]) for f in frames]
        bt.upload(held, row)
        refused(b, 0, 1, p, stride, w * 4 - 16, RGBA_F32, "a pitch below the f32 row bytes, again")
        for i in range(4): compare_frame(bt.frame(i, row), held[i], "behind refused calls, frame %d" % i)
        # the smallest pitch and stride are served
        tight = Source(frames, w, h, RGBA_F32, False)
        assert L.cfhd_amd_batch_upload_device_planar(b, 0, 4, tight.at(0), 4 * h * w * 4, w * 4, RGBA_F32) == 0, amd_last_error()
        # a pass in flight refuses
        assert L.cfhd_amd_batch_submit(b) == 0, amd_last_error()
        try:
            assert "flight" in refused(b, 0, 1, p, stride, pitch, RGBA_F32, "a pass in flight")
        finally:
            total = L.cfhd_amd_batch_wait(b)
        assert total > 0, (total, amd_last_error())
        want = [collected(f, "b64a", RGBA_F32) for f in frames]
        for i in range(4): compare_frame(bt.frame(i, row), want[i], "behind the pass, frame %d" % i)
        tight.unchanged("gates, the tight source")
    src.unchanged("gates")


# ---- 9. the kernels' times and names (hardware)
def check_kernel_times():
    w, h = SHAPE
    L = lib()
    samples = case_samples("4444", w, h)
    q = DQ.Queue(samples[0], "BGRA", FULL, 8)
    try:
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        d = Delivery(q, "BGRA", RGBA_F16, False, 8); d.set()
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        ms, name = L.cfhd_amd_decode_batch_kernel_ms(q.b, 9), L.cfhd_amd_decode_batch_kernel_name(q.b, 9)
        print("k_dec_deliver_rgba, 8 pictures of %d x %d: %.4f ms" % (w, h, ms))
        assert ms > 0 and name == DELIVER, (ms, name)
        packed = DP.Delivery(q, PACKED, False, 8); packed.set()
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) > 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
    finally:
        q.close()
    frames = [elements(p, RGBA_F32, 65535) for p in frame_planes("b64a", w, h)]
    src = Source(frames, w, h, RGBA_F32, False)
    row = row_bytes("b64a", w)
    mem = DeviceArray(np.concatenate([collected(f, "b64a", RGBA_F32).reshape(-1) for f in frames]))
    with Batch(intra("b64a", "4444"), w, h, 4) as bt, Batch(PF.RG48_444, w, h, 4) as rgb:
        assert L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT and L.cfhd_amd_batch_kernel_name(rgb.b, 20) == b"k_enc_collect"
        src.feed(bt.L, bt.b, 0, 2); src.feed(bt.L, bt.b, 2, 2)
        first = bt.run()
        ms = L.cfhd_amd_batch_kernel_ms(bt.b, 20)
        print("k_enc_collect_rgba, two launches of two frames: %.4f ms" % ms)
        assert ms > 0 and L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT, ms
        for i in range(4): assert L.cfhd_amd_batch_upload_device(bt.b, i, mem.ptr + i * row * h, row) == 0, amd_last_error()
        bt.run()
        assert L.cfhd_amd_batch_kernel_ms(bt.b, 20) == 0, "a pass fed by upload_device has no collect time"
        assert len(set(first)) == 4


# ---- 10. a torch tensor (hardware)
def check_torch(torch):
    """Delivery into a torch tensor (N, 4, H, W) through its data_ptr(), against numpy; and the tensor back into a frame batch."""
    w, h = SHAPE
    samples = case_samples("4444", w, h)
    for fmt, layout, dtype in (("BGRA", RGBA_U8, torch.uint8), ("BGRa", RGBA_F16, torch.float16), ("b64a", RGBA_F32, torch.float32)):
        q = DQ.Queue(samples[0], fmt, FULL, 8)
        try:
            t = torch.zeros((8, 4, h, w), dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            E = ELEMENT[layout]
            assert lib().cfhd_amd_decode_batch_set_device_pictures(q.b, t.data_ptr(), 4 * h * w * E, w * E, layout) == 0, amd_last_error()
            assert DP.run_pass(q, samples) == (8, [0] * 8)
            want = q.pictures(8)
            got = t.cpu().numpy()
            for i in range(8): assert np.array_equal(np.ascontiguousarray(got[i]).view(np.uint8).reshape(4, h, w * E), planes_of(want[i], w, h, fmt, layout)), "%s %s: picture %d" % (fmt, LAYOUT_NAMES[layout], i)
            with Batch(intra(fmt, "4444"), w, h, 8) as bt:
                assert bt.L.cfhd_amd_batch_upload_device_planar(bt.b, 0, 8, t.data_ptr(), 4 * h * w * E, w * E, layout) == 0, amd_last_error()
                for i in range(8): compare_frame(bt.frame(i, row_bytes(fmt, w)), want[i].reshape(h, -1), "%s %s: the tensor back in the frame queue, frame %d" % (fmt, LAYOUT_NAMES[layout], i))
        finally:
            q.close()
