"""BYR4 mosaics as four planar component tensors in device memory, on both queues: cfhd_amd_decode_batch_set_device_pictures with CFHD_AMD_PICTURES_BAYER_U16 / _F16 /
_F32 on a Bayer decode batch (k_dec_deliver_bayer: the mosaic of W x H photosites as four planes of H/2 rows of W/2 elements, plane k = 2 * (row & 1) + (column & 1))
and cfhd_amd_batch_upload_device_planar with CFHD_AMD_FRAMES_BAYER_* on every batch whose input is BYR4 (k_enc_collect_bayer, the mirror image).  The helpers and test
bodies shared by tests/test_gpu_bayer_planes.py (hardware) and tests/test_bayer_planes_emulated.py (the same functions inside cfhd_testlib.emulated_product(), where a
device pointer is a host pointer).

Every comparison is exact.  The witness of a decoded mosaic is ONE CFHD_DecodeSample handle fed the same samples (bayer_queue.witness); the element rules are the RG48
ones, stated in numpy by device_pictures.planar_bytes (delivery: u16 w, f32 w.astype(float32) * (float32(1) / float32(65535)), f16 that .astype(float16), compared as
bit patterns) and planar_frames.expected_words (collection: one single multiply, NaN to 0, clamp, round to nearest even) -- elements() below is planar_bytes' statement
on an array of any shape, and rule_is_planar_bytes() holds it to planar_bytes on all 65 536 words.  Device buffers are checked whole: filled with a pattern, guards in
front and behind, and afterwards equal to the pattern with exactly the row bytes of the planes replaced (deliveries) or byte for byte what they were (sources).

Mosaic sizes: 192 x 96 (planes 96 x 48: 12 lanes a row, a partial wave), 1008 x 244 (planes 504 x 122: 63 lanes, 122 quad rows are no multiple of the four waves of a
workgroup), and, for the delivery body and the geometry bodies of the frame queue, 1040 x 40 (planes 520 x 20: 65 groups of eight, the lane loop of either kernel makes
a second trip; its samples come from the library's own encoder).
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import device_pictures as DP
import planar_frames as PF
import bayer_queue as BQ
from device_pictures import DeviceArray, pattern, GUARD, mask_clock
from decode_queue import use_emulated, V, FULL
from bayer_queue import BYR4, BYR5

BAYER_U16, BAYER_F16, BAYER_F32 = 4, 5, 6
LAYOUTS = [BAYER_U16, BAYER_F16, BAYER_F32]
LAYOUT_NAMES = {BAYER_U16: "u16", BAYER_F16: "f16", BAYER_F32: "f32"}
LAYOUT_IDS = [LAYOUT_NAMES[l] for l in LAYOUTS]
ELEMENT = {BAYER_U16: 2, BAYER_F16: 2, BAYER_F32: 4}
RULE = {BAYER_U16: DP.PLANAR_U16, BAYER_F16: DP.PLANAR_F16, BAYER_F32: DP.PLANAR_F32}      # the RG48 layout whose element rule a Bayer layout shares
SHAPES = [(192, 96), (1008, 244)]
LONG = (1040, 40)
GEOMETRY_SHAPES = SHAPES + [LONG]
FILMSCAN2 = PF.FILMSCAN2
DELIVER, COLLECT = b"k_dec_deliver_bayer", b"k_enc_collect_bayer"


def lib():
    BQ.lib()
    return PF.lib()


# ---- the two views of a mosaic, and the delivery rule on an array of any shape
def elements(words, layout):
    """uint16 [..., n] photosite words -> the elements of `layout` by the delivery rule, uint8 [..., n * element size] (device_pictures.planar_bytes' statement)."""
    words = np.ascontiguousarray(words, np.uint16)
    if layout == BAYER_U16: return words.view(np.uint8)
    f32 = words.astype(np.float32) * (np.float32(1) / np.float32(65535))
    assert f32.dtype == np.float32
    if layout == BAYER_F32: return np.ascontiguousarray(f32).view(np.uint8)
    return np.ascontiguousarray(f32.astype(np.float16)).view(np.uint8)


_rule_checked = []


def rule_is_planar_bytes():
    """elements() against device_pictures.planar_bytes on an RG48 picture that holds every word in every component."""
    if _rule_checked: return
    every = np.arange(65536, dtype=np.uint16)
    picture = np.ascontiguousarray(np.repeat(every, 3)).view(np.uint8)
    for layout in LAYOUTS:
        want = DP.planar_bytes(picture, 256, 256, RULE[layout])
        for c in range(3): assert np.array_equal(want[c].reshape(-1), elements(every, layout)), LAYOUT_NAMES[layout]
    _rule_checked.append(True)


def quad_planes(mosaic, w, h):
    """A mosaic (w x h 16-bit photosites, any dtype view) -> uint16 [4, h/2, w/2]: plane k = 2 * (row & 1) + (column & 1)."""
    m = np.ascontiguousarray(mosaic).reshape(-1).view(np.uint16).reshape(h, w)
    return np.ascontiguousarray(np.stack([m[0::2, 0::2], m[0::2, 1::2], m[1::2, 0::2], m[1::2, 1::2]]))


def planes_of(mosaic, w, h, layout):
    """The four planes of a mosaic in the element type of `layout` by the delivery rule: uint8 [4, h/2, (w/2) * element size]."""
    rule_is_planar_bytes()
    return elements(quad_planes(mosaic, w, h), layout)


def mosaic_of(words):
    """uint16 [4, h/2, w/2] -> the mosaic, uint8 [h, 2 w]."""
    _, h2, w2 = words.shape
    m = np.empty((2 * h2, 2 * w2), np.uint16)
    m[0::2, 0::2], m[0::2, 1::2], m[1::2, 0::2], m[1::2, 1::2] = words[0], words[1], words[2], words[3]
    return m.view(np.uint8)


def collected(planes, layout):
    """Planes of elements (uint8 [4, h/2, row bytes]) -> the mosaic the collection rule gives, uint8 [h, 2 w] (planar_frames.expected_words on every plane)."""
    return mosaic_of(PF.expected_words(planes, RULE[layout]))


def geometry(w, h, layout, padded):
    """(row bytes, pitch, stride) of the planes of a w x h mosaic: the contiguous (n, 4, h/2, w/2) tensor, or a pitch of row bytes + 48 and a stride of four planes + 4096."""
    row = (w // 2) * ELEMENT[layout]
    assert row % 16 == 0
    pitch = row + (48 if padded else 0)
    return row, pitch, 4 * (h // 2) * pitch + (4096 if padded else 0)


class Delivery(DP.Delivery):
    """device_pictures.Delivery for the four planes of the mosaics of a Bayer decode batch."""
    def __init__(self, q, layout, padded, npictures):
        self.q, self.layout = q, layout
        self.row, self.pitch, self.stride = geometry(q.w, q.h, layout, padded)
        self.image = pattern(GUARD + npictures * self.stride + GUARD)
        self.mem = DeviceArray(self.image)

    def expect(self, pictures):
        h2 = self.q.h // 2
        for i, p in enumerate(pictures):
            if p is None: continue
            at = GUARD + i * self.stride
            self.image[at: at + 4 * h2 * self.pitch].reshape(4 * h2, self.pitch)[:, : self.row] = planes_of(p, self.q.w, self.q.h, self.layout).reshape(4 * h2, self.row)
        return self.image


class Source(PF.Source):
    """planar_frames.Source for frames of four planes (each uint8 [4, h/2, (w/2) * element size]) of w x h mosaics."""
    def __init__(self, frames, w, h, layout, padded):
        self.w, self.h, self.layout, self.n = w, h, layout, len(frames)
        self.row, self.pitch, self.stride = geometry(w, h, layout, padded)
        self.image = pattern(GUARD + self.n * self.stride + GUARD)
        for i, f in enumerate(frames):
            at = GUARD + i * self.stride
            self.image[at: at + 2 * h * self.pitch].reshape(2 * h, self.pitch)[:, : self.row] = np.asarray(f).reshape(2 * h, self.row)
        self.mem = DeviceArray(self.image)


class Batch(PF.Batch):
    """planar_frames.Batch with cfhd_amd_batch_create_bayer among the constructors.  kind: (entry, pixel format, encoded format, flags, quality)."""
    def __init__(self, kind, w, h, n, mode=1):
        if kind[0] != "bayer": PF.Batch.__init__(self, kind, w, h, n, mode); return
        entry, pix, encoded, flags, quality = kind
        self.L = L = lib(); self.w, self.h, self.n, self.mode = w, h, n, mode
        L.cfhd_amd_set_clip_guid(DP.GUID)
        self.b = L.cfhd_amd_batch_create_bayer(w, h, pix, flags, quality, n, 1, mode)
        assert self.b, "cfhd_amd_batch_create_bayer -> NULL (%s)" % amd_last_error()


EX = ("ex", BYR4, ENCODED_BAYER, 0, QUALITY_FILMSCAN1)


def compare_mosaic(got, want, what):
    PF.compare_frame(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


def source_of(w, h):
    """The reference's samples where oracle/_ref is built, the product's otherwise; the long shape always from the library's own encoder."""
    return "amd" if (w, h) == LONG else DP.source()


# ---- 1. delivery equals numpy
def check_delivery(w, h, layout):
    source = source_of(w, h)
    samples = BQ.samples_of(w, h, source)
    want, geo = BQ.witness(w, h, source)
    BQ.assert_clamps_reached(want, "%d x %d" % (w, h))
    if (w, h) == LONG: assert (w // 2) // 8 == 65              # (a lane of k_dec_deliver_bayer makes a second trip)
    q = BQ.Queue(samples[0], 8)
    try:
        assert (q.w, q.h, q.row_bytes) == geo == (w, h, 2 * w)
        # the fused last level into the contiguous tensor, the pair into a pitch with padding
        for (mode, name), padded in zip(BQ.ROUTES, (False, True)):
            with BQ.inverse(mode):
                d = Delivery(q, layout, padded, 8)
                if not padded: assert d.pitch == (w // 2) * ELEMENT[layout] and d.stride == 4 * (h // 2) * d.pitch      # a contiguous (8, 4, H/2, W/2) tensor
                d.set()
                ret, status = DP.run_pass(q, samples)
                assert ret == 8 and status == [0] * 8, (mode, ret, status, amd_last_error())
                assert q.last_level() == name, (mode, q.last_level())
                d.check(want, "%d x %d, %s, %s, %s" % (w, h, LAYOUT_NAMES[layout], mode, "pitch with padding" if padded else "contiguous tensor"))
                for i, p in enumerate(q.pictures(8)): assert np.array_equal(p, want[i]), "download_output(%d) beside device delivery" % i
    finally:
        q.close()


# ---- 2. nothing else is touched; switching back to PACKED and to NULL
def check_short_pass_and_switching(layout):
    w, h = SHAPES[0]
    samples = BQ.samples_of(w, h, DP.source())
    want, _ = BQ.witness(w, h, DP.source())
    q = BQ.Queue(samples[0], 8)
    L = lib()
    try:
        d = Delivery(q, layout, True, 8)
        assert d.pitch > d.row and d.stride > 4 * (h // 2) * d.pitch
        d.set()
        ret, status = DP.run_pass(q, samples, count=3)
        assert (ret, status) == (3, [0] * 3)
        d.check(want[:3] + [None] * 5, "count = 3 of 8: planes, padding, gaps, the pictures behind the count, the guards")
        # back to PACKED between passes: the planes' buffer is left alone, the packed one gets the mosaics
        packed = DP.Delivery(q, DP.PACKED, True, 8); packed.set()
        ret, status = DP.run_pass(q, samples[5:8])
        assert (ret, status) == (3, [0] * 3)
        packed.check(want[5:8] + [None] * 5, "PACKED behind a BAYER layout")
        d.check([None] * 8, "the planes while PACKED is set")
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        # to NULL: neither buffer is touched, the pictures are in the batch
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check([None] * 8, "the planes after set_device_pictures(NULL)"); packed.check([None] * 8, "the packed buffer after set_device_pictures(NULL)")
        for i, p in enumerate(q.pictures(8)): assert np.array_equal(p, want[i])
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        # and the planes again, the whole batch
        d.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check(want, "count = 8 behind PACKED and NULL")
    finally:
        q.close()


# ---- 3. verdicts
def check_verdicts(layout):
    """bayer_queue.check_verdicts' pass -- an intact sample, a sample cut in half, a damaged code stream (which sends every sample the parser passed through the handle
    inside wait), a mosaic of another size, a 4:2:2 sample the parser refuses, an intact sample --: the planes agree with status[i]."""
    w, h = SHAPES[0]
    good = BQ.samples_of(w, h, "amd")
    ow, oh = 208, 104
    other = amd_encode_frames([synth_bayer(ow, oh, 5).reshape(-1).view(np.uint8).copy()], ow * 2, ow, oh, BYR4, ENCODED_BAYER)[0]
    yuv = DQ.samples_of("422", 192, 96, "amd", n=2)[0]
    samples = [good[0], good[1], BQ.damaged_stream(good[BQ.NOISE]), other, yuv, good[5]]
    sizes = [len(s) for s in samples]; sizes[1] = (len(good[1]) // 2) & ~3
    res, _ = DQ.handle_pictures(samples, "BYR4", FULL, sizes=sizes)
    codes = [rc for rc, _ in res]
    print("the handle answers", codes)
    assert codes[0] == 0 and codes[5] == 0 and all(codes[1:5]), codes
    handle = [p if rc == 0 else np.zeros(2 * w * h, np.uint8) for rc, p in res]
    for rc, p in res:
        if rc: assert not p.any()                              # (the handle zero-fills what it refuses)
    assert handle[0].any() and handle[5].any()
    q = BQ.Queue(good[0], 8)
    try:
        d = Delivery(q, layout, True, 8); d.set()
        blob, offsets, _ = DQ.pack(samples)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        ret, status = q.wait(len(samples))
        assert status == codes and ret == 2, (status, codes)
        # a failed sample: zeros (0.0 in every element type) in all four planes; the samples the handle decoded inside wait: the handle's pictures
        d.check(handle + [None, None], "verdicts, %s" % LAYOUT_NAMES[layout])
        for i, p in enumerate(q.pictures(6)): assert np.array_equal(p, handle[i]), "download_output(%d)" % i
        # an intact pass on the same batch and buffer afterwards
        ret, status = DP.run_pass(q, good)
        assert ret == 8 and status == [0] * 8
        d.check(BQ.witness(w, h, "amd")[0], "an intact pass behind the damaged one, %s" % LAYOUT_NAMES[layout])
    finally:
        q.close()


# ---- 4. collection equals numpy
RULE_W, RULE_H, RULE_N = 192, 96, 4
RULE_ELEMENTS = RULE_N * 4 * (RULE_W // 2) * (RULE_H // 2)


def rule_frames(layout):
    """Four frames of four planes of 96 x 48 elements (73 728 in all).  U16 and F16: i * 40503 mod 65536 over consecutive i -- every one of the 65 536 words, every
    binary16 pattern.  F32: the exact ties of planar_frames.f32_rule_values() (65 537 products of the one single multiply that end in .5), its specials, then its
    random patterns."""
    assert RULE_ELEMENTS == 73728
    if layout != BAYER_F32:
        bits = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 40503) & 0xffff).astype(np.uint16)
        assert np.unique(bits).size == 65536
        flat = bits.view(np.uint8)
    else:
        values = PF.f32_rule_values()
        near, specials, rest = values[:196605], values[196605: 196605 + 13], values[196605 + 13:]
        prod = (near * np.float32(65535)).astype(np.float64)
        ties = near[(prod - np.floor(prod)) == 0.5]
        assert ties.size == 65537 and np.isnan(specials).sum() == 4 and np.isinf(specials).sum() == 2
        flat = np.concatenate([ties, specials, rest[: RULE_ELEMENTS - ties.size - specials.size]]).astype(np.float32).view(np.uint8)
    return list(np.ascontiguousarray(flat).reshape(RULE_N, 4, RULE_H // 2, (RULE_W // 2) * ELEMENT[layout]))


def check_collection(layout):
    w, h, n = RULE_W, RULE_H, RULE_N
    frames = rule_frames(layout)
    with Batch(EX, w, h, n) as bt:
        src = Source(frames, w, h, layout, False)
        assert src.pitch == (w // 2) * ELEMENT[layout] and src.stride == 4 * (h // 2) * src.pitch      # a contiguous (4, 4, H/2, W/2) tensor
        src.feed(bt.L, bt.b, 0, n)
        seen = []
        for i in range(n):
            want = collected(frames[i], layout)
            seen.append(want.view(np.uint16).reshape(-1))
            compare_mosaic(bt.frame(i, 2 * w), want, "%s, frame %d" % (LAYOUT_NAMES[layout], i))
        if layout == BAYER_U16: assert np.unique(np.concatenate(seen)).size == 65536
        if layout == BAYER_F16:
            words = PF.expected_words(np.arange(65536, dtype=np.uint16).view(np.uint8), DP.PLANAR_F16)
            assert words[0x03ff] == 4 and words[0x3c00] == 65535 and words[0x7e00] == 0 and words[0xfc00] == 0 and words[0x7c00] == 65535
        src.unchanged(LAYOUT_NAMES[layout])


# ---- 5. inversion
def all_words_mosaics():
    """Four 192 x 96 mosaics (73 728 photosites) that hold every one of the 65 536 words."""
    words = ((np.arange(RULE_ELEMENTS, dtype=np.uint32) * 40503 + 977) & 0xffff).astype(np.uint16)
    assert np.unique(words).size == 65536
    return list(words.view(np.uint8).reshape(RULE_N, RULE_H, 2 * RULE_W))


def check_inversion(layout):
    """collect(deliver(w)) = w for all 65 536 words through U16 and F32; through F16, delivering what was collected returns every delivered bit pattern."""
    w, h, n = RULE_W, RULE_H, RULE_N
    mosaics = all_words_mosaics()
    planes = [planes_of(m, w, h, layout) for m in mosaics]
    with Batch(EX, w, h, n) as bt:
        src = Source(planes, w, h, layout, False)
        src.feed(bt.L, bt.b, 0, n)
        for i in range(n):
            got = bt.frame(i, 2 * w)
            if layout != BAYER_F16: compare_mosaic(got, mosaics[i], "%s of the delivered mosaic %d" % (LAYOUT_NAMES[layout], i))
            else: assert np.array_equal(planes_of(got, w, h, layout), planes[i]), "f16: mosaic %d delivered, collected and delivered again" % i
    if layout == BAYER_F16:                                    # the planes held every bit pattern F16 delivery can make
        every = np.unique(elements(np.arange(65536, dtype=np.uint16), BAYER_F16).view(np.uint16))
        assert np.array_equal(np.unique(np.concatenate([p.view(np.uint16).reshape(-1) for p in planes])), every)


# ---- 6. runs and geometry
def geometry_frames(w, h, layout):
    """Four mosaics' planes -- a synth_bayer mosaic, the noise mosaic, the checker mosaic, a synth_bayer mosaic -- by the delivery rule."""
    return [planes_of(m, w, h, layout) for m in BQ.mosaics(w, h)[1:5]]


def check_runs(w, h, layout):
    frames = geometry_frames(w, h, layout)
    want = [collected(f, layout) for f in frames]
    assert len(set(x.tobytes() for x in want)) == 4
    if (w, h) == LONG: assert (w // 2) // 8 == 65
    for padded in (False, True):
        what = "%dx%d, %s, %s" % (w, h, LAYOUT_NAMES[layout], "pitch with padding" if padded else "contiguous tensor")
        src = Source(frames, w, h, layout, padded)
        if padded: assert src.pitch == src.row + 48 and src.stride == 4 * (h // 2) * src.pitch + 4096
        if not padded:
            with Batch(EX, w, h, 4) as bt:
                for first, count in ((1, 2), (0, 1), (3, 1)): src.feed(bt.L, bt.b, first, count)
                for i in range(4): compare_mosaic(bt.frame(i, 2 * w), want[i], "%s, frame %d" % (what, i))
        # frames 1 - 2 alone, over frames cfhd_amd_batch_upload put there
        held = [np.ascontiguousarray(want[(i + 2) % 4][::-1]) for i in range(4)]
        with Batch(EX, w, h, 4) as bt:
            bt.upload(held, 2 * w)
            src.feed(bt.L, bt.b, 1, 2)
            for i in range(4): compare_mosaic(bt.frame(i, 2 * w), want[i] if i in (1, 2) else held[i], "%s, frames 1 - 2 over uploaded frames, frame %d" % (what, i))
        src.unchanged(what)


# ---- 7. every kind of BYR4 batch
# (cfhd_amd_batch_create_bayer refuses the qualities whose tables move; cfhd_amd_batch_create_stream is the entry that takes them.  "chunks": an intra batch cut into
# chunks with streams of their own -- CFHD_AMD_CHUNK=3: frames 0 - 2 | 3 --, a run that crosses the cut is split per chunk)
KINDS = {"ex-mode1": (EX, 1, None), "bayer-mode1": (("bayer", BYR4, 0, 0, QUALITY_FILMSCAN1), 1, None), "bayer-mode0": (("bayer", BYR4, 0, 0, QUALITY_FILMSCAN1), 0, None),
         "stream-filmscan2": (("stream", BYR4, ENCODED_BAYER, 0, FILMSCAN2), 1, None), "chunks": (EX, 1, "3")}
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
        kind, mode, chunk = KINDS[name]
        with chunked(chunk), Batch(kind, w, h, 4, mode) as bt:
            bt.upload(frames, 2 * w)
            samples = bt.run()
            _host_fed[key] = (samples, bt.outputs(2 * w) if mode == 0 else None)
    return _host_fed[key]


def check_kind(name, layout):
    assert layout in (BAYER_U16, BAYER_F32)
    w, h = SHAPES[0]
    kind, mode, chunk = KINDS[name]
    frames = [np.asarray(m).reshape(h, 2 * w) for m in BQ.mosaics(w, h)[:4]]
    if name == "stream-filmscan2": assert lib().cfhd_amd_quantizer_is_static(w, h, BYR4, ENCODED_BAYER, 0, FILMSCAN2) == 0, "the tables of this stream move"
    first, first_out = host_fed(name, w, h, frames)
    assert len(set(first)) == 4
    src = Source([planes_of(f, w, h, layout) for f in frames], w, h, layout, True)
    with chunked(chunk), Batch(kind, w, h, 4, mode) as bt:
        assert bt.L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT
        if chunk: src.feed(bt.L, bt.b, 1, 3); src.feed(bt.L, bt.b, 0, 1)
        else: src.feed(bt.L, bt.b, 0, 4)
        for i in range(4): compare_mosaic(bt.frame(i, 2 * w), frames[i], "%s: frame %d in front of the pass" % (name, i))
        second = bt.run()
        if name == "stream-filmscan2":
            stats = (ctypes.c_int * 3)()
            assert bt.L.cfhd_amd_batch_stream_stats(bt.b, stats) == 0
            print("%s: %d rounds, %d frames coded, %d units whose tables moved" % (name, stats[0], stats[1], stats[2]))
        for i in range(4): assert second[i] == first[i], "%s, %s: sample %d of the batch fed from planes differs (%d / %d bytes)" % (name, LAYOUT_NAMES[layout], i, len(second[i]), len(first[i]))
        if mode == 0:
            for i, o in enumerate(bt.outputs(2 * w)): assert np.array_equal(o, first_out[i]), "%s, %s: mosaic %d of the batch fed from planes differs" % (name, LAYOUT_NAMES[layout], i)
        for i in range(4): compare_mosaic(bt.frame(i, 2 * w), frames[i], "%s: frame %d behind the pass" % (name, i))
    src.unchanged(name)


# ---- 8. the chain, all in HBM: Bayer decode queue -> planes -> frame queue
def check_chain(layout):
    assert layout in (BAYER_U16, BAYER_F32)
    w, h = SHAPES[0]
    samples = BQ.samples_of(w, h, DP.source())
    want, _ = BQ.witness(w, h, DP.source())
    q = BQ.Queue(samples[0], 8)
    try:
        d = Delivery(q, layout, True, 8); d.set()
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        def device_feed(L, b):
            lib()
            assert L.cfhd_amd_batch_upload_device_planar(b, 0, 8, d.mem.ptr + GUARD, d.stride, d.pitch, layout) == 0, amd_last_error()
        chained = DP.encode_batch(BYR4, ENCODED_BAYER, 0, w, h, 8, device_feed)
    finally:
        q.close()
    def host_feed(L, b):
        for i in range(8): assert L.cfhd_amd_batch_upload(b, i, np.ascontiguousarray(want[i]).ctypes.data_as(V), 2 * w) == 0
    direct = DP.encode_batch(BYR4, ENCODED_BAYER, 0, w, h, 8, host_feed)
    assert len(set(direct)) == 8
    for i in range(8): assert chained[i] == direct[i], "%s: sample %d of the chain differs from the sample of the handle's mosaic uploaded from the host" % (LAYOUT_NAMES[layout], i)


# ---- 9. gates
def check_decode_gates():
    w, h = SHAPES[0]
    w2, h2 = w // 2, h // 2
    L = lib()
    bayer = BQ.samples_of(w, h, "amd")
    yuv = DQ.samples_of("422", w, h, "amd", n=2)
    q = BQ.Queue(bayer[0], 8); yu64 = DQ.Queue(yuv[0], "YU64", FULL, 2); rg48 = DQ.Queue(yuv[0], "RG48", FULL, 2)
    try:
        d = Delivery(q, BAYER_F32, True, 8)
        p, stride, pitch = d.mem.ptr + GUARD, d.stride, d.pitch
        def refused(queue, ptr, s, pt, layout, what):
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, ptr, s, pt, layout) == -1, what
            text = amd_last_error()
            assert text and "decode queue" in text, "%s: refused without a text (%r)" % (what, text)
            return text
        # a BAYER layout on any other batch -- the refusals existing tests pin, asserted here too: layout 4 on a YU64 batch, layouts 1 .. 3 on a Bayer batch
        elsewhere = set(refused(b, p, stride, pitch, layout, "layout %d on a batch that is no Bayer batch" % layout) for b in (yu64, rg48) for layout in LAYOUTS)
        assert len(elsewhere) == 1 and elsewhere == {refused(yu64, p, stride, pitch, -1, "a negative layout")}, elsewhere
        rgb = set(refused(q, p, stride, pitch, layout, "PLANAR layout %d on a Bayer batch" % layout) for layout in (DP.PLANAR_U16, DP.PLANAR_F16, DP.PLANAR_F32))
        assert len(rgb) == 1 and "RG48" in list(rgb)[0], rgb
        unknown = refused(q, p, stride, pitch, 7, "layout 7 on a Bayer batch")
        assert {unknown} == elsewhere
        low_pitch = set(refused(q, p, stride, w2 * ELEMENT[layout] - 16, layout, "a pitch below (W/2) x element size, %s" % LAYOUT_NAMES[layout]) for layout in LAYOUTS)
        low_pitch.add(refused(q, p, stride, -pitch, BAYER_F32, "a negative pitch"))
        low_stride = set(refused(q, p, pt * (4 * h2 - 1) + w2 * ELEMENT[layout] - 16, pt, layout, "a stride below four planes, %s" % LAYOUT_NAMES[layout])
                         for layout, pt in ((BAYER_U16, pitch), (BAYER_F16, w2 * 2), (BAYER_F32, pitch)))
        off = set([refused(q, p + 8, stride, pitch, BAYER_F32, "a pointer off 16"), refused(q, p, stride + 8, pitch, BAYER_F32, "a stride off 16"), refused(q, p, stride, pitch + 8, BAYER_F32, "a pitch off 16")])
        assert len(low_pitch) == 1 and len(low_stride) == 1 and len(off) == 1
        assert len(elsewhere | rgb | low_pitch | low_stride | off) == 5, "the texts of the refusals are distinct"
        # the smallest pitch and stride are served
        for layout in LAYOUTS:
            row = w2 * ELEMENT[layout]
            assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, p, row * (4 * h2 - 1) + row, row, layout) == 0, amd_last_error()
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, p, pitch * (4 * h2 - 1) + w2 * 4, pitch, BAYER_F32) == 0, amd_last_error()
        # a refusal leaves the layout that was set in place, and nothing was launched: the memory holds what was there
        refused(q, p, stride, w2 * 4 - 16, BAYER_F32, "a pitch below the row bytes, again")
        d.check([None] * 8, "behind refused calls")
        # a pass in flight refuses
        d.set()
        blob, offsets, sizes = DQ.pack(bayer)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        try:
            assert "flight" in refused(q, p, stride, pitch, BAYER_F32, "a pass in flight")
            assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == -1 and amd_last_error()
        finally:
            ret, status = q.wait(8)
        assert ret == 8 and status == [0] * 8
        d.check(BQ.witness(w, h, "amd")[0], "the pass the refused calls were made in")
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER and L.cfhd_amd_decode_batch_kernel_name(yu64.b, 9) == b"k_dec_deliver"
    finally:
        q.close(); yu64.close(); rg48.close()


def check_frame_gates():
    w, h = SHAPES[0]
    w2, h2 = w // 2, h // 2
    L = lib()
    frames = geometry_frames(w, h, BAYER_F32)
    src = Source(frames, w, h, BAYER_F32, True)
    p, stride, pitch = src.at(0), src.stride, src.pitch
    def refused(b, first, count, ptr, s, pt, layout, what):
        assert L.cfhd_amd_batch_upload_device_planar(b, first, count, ptr, s, pt, layout) == -1, what
        text = amd_last_error()
        assert text and "planar" in text, "%s: refused without a text (%r)" % (what, text)
        return text
    with Batch(("bayer", BYR5, 0, 0, QUALITY_FILMSCAN1), w, h, 4) as byr5:
        t_byr5 = set(refused(byr5.b, 0, 1, p, stride, pitch, layout, "a BYR5 batch, layout %d" % layout) for layout in LAYOUTS + [DP.PLANAR_U16])
    with Batch(PF.RG48_444, w, h, 4) as rg48:
        # (layout 4 on an RG48 batch: what tests/planar_frames.py pins as its unknown layout)
        t_rg48 = set(refused(rg48.b, 0, 1, p, stride, pitch, layout, "layout %d on an RG48 batch" % layout) for layout in LAYOUTS)
    with Batch(("ex", PIX_YUY2, ENCODED_YUV422, 0, QUALITY_FILMSCAN1), w, h, 4) as yuy2:
        t_yuy2 = set(refused(yuy2.b, 0, 1, p, stride, pitch, layout, "layout %d on a YUY2 batch" % layout) for layout in LAYOUTS)
        assert "RG48" in refused(yuy2.b, 0, 1, p, stride, pitch, DP.PLANAR_U16, "PLANAR_U16 on a YUY2 batch")
    with Batch(EX, w, h, 4) as bt:
        b = bt.b
        t_rgb = set(refused(b, 0, 1, p, stride, pitch, layout, "layout %d on a BYR4 batch" % layout) for layout in (DP.PLANAR_U16, DP.PLANAR_F16, DP.PLANAR_F32, 0, 7, -1))
        t_negative = refused(b, 0, 1, p, stride, -pitch, BAYER_F32, "a negative pitch")
        t_low = set(refused(b, 0, 1, p, stride, w2 * ELEMENT[layout] - 16, layout, "a pitch below (W/2) x element size, %s" % LAYOUT_NAMES[layout]) for layout in LAYOUTS)
        t_stride = set(refused(b, 0, 2, p, 4 * h2 * pt - 16, pt, layout, "a stride below four planes, %s" % LAYOUT_NAMES[layout]) for layout, pt in ((BAYER_U16, pitch), (BAYER_F16, w2 * 2), (BAYER_F32, pitch)))
        assert refused(b, 0, 2, p, 3 * h2 * pitch, pitch, BAYER_F32, "a stride of three planes") in t_stride
        t_off = set([refused(b, 0, 1, p + 8, stride, pitch, BAYER_F32, "a pointer off 16"), refused(b, 0, 2, p, stride + 8, pitch, BAYER_F32, "a stride off 16"), refused(b, 0, 1, p, stride, pitch + 8, BAYER_F32, "a pitch off 16")])
        t_run = set([refused(b, 0, 0, p, stride, pitch, BAYER_F32, "count 0"), refused(b, 3, 2, p, stride, pitch, BAYER_F32, "a run that leaves the batch"), refused(b, -1, 1, p, stride, pitch, BAYER_F32, "a run in front of the batch")])
        t_null = refused(b, 0, 1, None, stride, pitch, BAYER_F32, "no pointer")
        for s in (t_byr5, t_rg48, t_yuy2, t_rgb, t_low, t_stride, t_off, t_run): assert len(s) == 1, s
        assert t_low == {t_negative}
        assert len(t_byr5 | t_rg48 | t_yuy2 | t_rgb | t_low | t_stride | t_off | t_run | {t_null}) == 9, "the texts of the refusals are distinct"
        # nothing was launched: the frames are what upload put there
        held = [np.ascontiguousarray(collected(f, BAYER_F32)[::-1]) for f in frames]
        bt.upload(held, 2 * w)
        refused(b, 0, 1, p, stride, w2 * 4 - 16, BAYER_F32, "a pitch below the f32 row bytes, again")
        for i in range(4): compare_mosaic(bt.frame(i, 2 * w), held[i], "behind refused calls, frame %d" % i)
        # the smallest pitch and stride are served
        tight = Source(frames, w, h, BAYER_F32, False)
        assert L.cfhd_amd_batch_upload_device_planar(b, 0, 4, tight.at(0), 4 * h2 * w2 * 4, w2 * 4, BAYER_F32) == 0, amd_last_error()
        # a pass in flight refuses
        assert L.cfhd_amd_batch_submit(b) == 0, amd_last_error()
        try:
            assert "flight" in refused(b, 0, 1, p, stride, pitch, BAYER_F32, "a pass in flight")
        finally:
            total = L.cfhd_amd_batch_wait(b)
        assert total > 0, (total, amd_last_error())
        want = [collected(f, BAYER_F32) for f in frames]
        for i in range(4): compare_mosaic(bt.frame(i, 2 * w), want[i], "behind the pass, frame %d" % i)
        tight.unchanged("gates, the tight source")
    src.unchanged("gates")


# ---- 11. the kernels' times and names (hardware)
def check_kernel_times():
    w, h = SHAPES[0]
    L = lib()
    samples = BQ.samples_of(w, h, "amd")
    want, _ = BQ.witness(w, h, "amd")
    q = BQ.Queue(samples[0], 8)
    try:
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        d = Delivery(q, BAYER_F16, False, 8); d.set()
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        ms, name = L.cfhd_amd_decode_batch_kernel_ms(q.b, 9), L.cfhd_amd_decode_batch_kernel_name(q.b, 9)
        print("k_dec_deliver_bayer, 8 mosaics of %d x %d: %.4f ms" % (w, h, ms))
        assert ms > 0 and name == DELIVER, (ms, name)
        packed = DP.Delivery(q, DP.PACKED, False, 8); packed.set()
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) > 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
    finally:
        q.close()
    frames = geometry_frames(w, h, BAYER_F32)
    src = Source(frames, w, h, BAYER_F32, False)
    mem = DeviceArray(np.concatenate([collected(f, BAYER_F32).reshape(-1) for f in frames]))
    with Batch(EX, w, h, 4) as bt, Batch(PF.RG48_444, w, h, 4) as rgb:
        assert L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT and L.cfhd_amd_batch_kernel_name(rgb.b, 20) == b"k_enc_collect"
        src.feed(bt.L, bt.b, 0, 2); src.feed(bt.L, bt.b, 2, 2)
        first = bt.run()
        ms = L.cfhd_amd_batch_kernel_ms(bt.b, 20)
        print("k_enc_collect_bayer, two launches of two frames: %.4f ms" % ms)
        assert ms > 0 and L.cfhd_amd_batch_kernel_name(bt.b, 20) == COLLECT, ms
        for i in range(4): assert L.cfhd_amd_batch_upload_device(bt.b, i, mem.ptr + i * 2 * w * h, 2 * w) == 0, amd_last_error()
        bt.run()
        assert L.cfhd_amd_batch_kernel_ms(bt.b, 20) == 0, "a pass fed by upload_device has no collect time"
        assert len(set(first)) == 4
