"""The frame queue fed from planar R, G, B tensors in device memory: cfhd_amd_batch_upload_device_planar (k_enc_collect: a run of frames out of u16 / f16 / f32 planes
into the batch's RG48 frame slots, one launch) and cfhd_amd_batch_download_frame (a frame as the batch holds it).  The helpers and test bodies shared by
tests/test_gpu_planar_frames.py (hardware) and tests/test_planar_frames_emulated.py (the same functions inside cfhd_testlib.emulated_product(), where a device pointer
is a host pointer).

Every comparison is exact.  The word expected of an element is numpy's, on float32 (float16 widened with .astype(float32)):
    t = x * float32(65535);  t = where(isnan(t), 0, t);  rint(clip(t, 0, 65535)).astype(uint16)
-- one single multiply, NaN to 0, clamp, round to nearest even.  A source buffer is checked whole: it is filled with a pattern, guards in front and behind, and after
the calls it has to be byte for byte what it was.  Test infrastructure only."""
import ctypes, os, subprocess
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import device_pictures as DP
from device_pictures import DeviceArray, pattern, GUARD, encode_batch, PLANAR_U16, PLANAR_F16, PLANAR_F32, ELEMENT, LAYOUT_NAMES
from decode_queue import use_emulated, V

LAYOUTS = [PLANAR_U16, PLANAR_F16, PLANAR_F32]
LAYOUT_IDS = [LAYOUT_NAMES[l] for l in LAYOUTS]
HIGH, FILMSCAN2 = 3, 5


def lib():
    L = DP.lib()
    if not getattr(L, "_planar_frames_declared", False):
        L.cfhd_amd_batch_upload_device_planar.argtypes = [V, ctypes.c_int, ctypes.c_int, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
        L.cfhd_amd_batch_download_frame.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_batch_download_output.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_batch_upload_device.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_batch_submit.argtypes = [V]
        L.cfhd_amd_batch_wait.restype = ctypes.c_longlong; L.cfhd_amd_batch_wait.argtypes = [V]
        L.cfhd_amd_batch_kernel_ms.restype = ctypes.c_float; L.cfhd_amd_batch_kernel_ms.argtypes = [V, ctypes.c_int]
        L.cfhd_amd_batch_kernel_name.restype = ctypes.c_char_p; L.cfhd_amd_batch_kernel_name.argtypes = [V, ctypes.c_int]
        four = [ctypes.c_int] * 4
        L.cfhd_amd_batch_create_stream.restype = V; L.cfhd_amd_batch_create_stream.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32] + four
        L.cfhd_amd_batch_create_groups.restype = V; L.cfhd_amd_batch_create_groups.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + four
        L.cfhd_amd_batch_create_group_stream.restype = V; L.cfhd_amd_batch_create_group_stream.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + four
        L.cfhd_amd_quantizer_is_static.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
        L.cfhd_amd_batch_stream_stats.argtypes = [V, ctypes.POINTER(ctypes.c_int)]
        L._planar_frames_declared = True
    return L


# ---- the rule, and the two views of a frame
def expected_words(planes, layout):
    """uint8 [..., row bytes] of elements in `layout` -> the RG48 words the rule gives, uint16 [..., width]."""
    if layout == PLANAR_U16: return np.ascontiguousarray(planes).view(np.uint16)
    x = np.ascontiguousarray(planes).view(np.float16).astype(np.float32) if layout == PLANAR_F16 else np.ascontiguousarray(planes).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = x * np.float32(65535)
        assert t.dtype == np.float32
        t = np.where(np.isnan(t), np.float32(0), t)
        return np.rint(np.clip(t, np.float32(0), np.float32(65535))).astype(np.uint16)


def packed_frame(words):
    """uint16 [3, h, w] (planes R, G, B) -> the RG48 frame, uint8 [h, 6 w]."""
    _, h, w = words.shape
    return np.ascontiguousarray(words.transpose(1, 2, 0)).view(np.uint8).reshape(h, 6 * w)


def planes_of(frame, w, h, layout):
    """A packed RG48 frame in the element type of `layout` by the DELIVERY rules (device_pictures.planar_bytes): uint8 [3, h, w * element size]."""
    return DP.planar_bytes(np.ascontiguousarray(frame).reshape(-1), w, h, layout)


class Source:
    """Planar frames (each uint8 [3, h, w * element size]) in device memory at a geometry: the contiguous tensor, or a pitch of row bytes (rounded up to 16) + 48 and a
    stride of frame + 4096; prefilled with the pattern, guards in front and behind."""
    def __init__(self, frames, w, h, layout, padded):
        self.w, self.h, self.layout, self.n = w, h, layout, len(frames)
        self.row = w * ELEMENT[layout]
        self.pitch = ((self.row + 15) & ~15) + (48 if padded else 0)
        self.stride = 3 * h * self.pitch + (4096 if padded else 0)
        self.image = pattern(GUARD + self.n * self.stride + GUARD)
        for i, f in enumerate(frames):
            at = GUARD + i * self.stride
            self.image[at: at + 3 * h * self.pitch].reshape(3 * h, self.pitch)[:, : self.row] = np.asarray(f).reshape(3 * h, self.row)
        self.mem = DeviceArray(self.image)

    def at(self, i): return self.mem.ptr + GUARD + i * self.stride

    def feed(self, L, b, first, count, src_first=None):
        """Frames first .. first + count - 1 of the batch from frames src_first .. of this buffer (default: the same indices)."""
        rc = L.cfhd_amd_batch_upload_device_planar(b, first, count, self.at(first if src_first is None else src_first), self.stride, self.pitch, self.layout)
        assert rc == 0, (rc, amd_last_error())

    def unchanged(self, what):
        assert np.array_equal(self.mem.read(), self.image), "%s: the source buffer was written to" % what


class Batch:
    """A frame-queue batch by any of the four constructors, destroyed on the way out.  kind: (entry, pixel format, encoded format, flags, quality)."""
    def __init__(self, kind, w, h, n, mode=1):
        entry, pix, encoded, flags, quality = kind
        self.L = L = lib(); self.w, self.h, self.n, self.mode = w, h, n, mode
        L.cfhd_amd_set_clip_guid(DP.GUID)
        if entry == "ex": self.b = L.cfhd_amd_batch_create_ex(w, h, pix, encoded, flags, quality, n, 1, mode)
        elif entry == "stream": self.b = L.cfhd_amd_batch_create_stream(w, h, pix, encoded, flags, quality, n, 1, mode)
        elif entry == "groups": self.b = L.cfhd_amd_batch_create_groups(w, h, pix, flags, quality, n, 1, mode)
        else: self.b = L.cfhd_amd_batch_create_group_stream(w, h, pix, flags, quality, n, 1, mode)
        assert self.b, "%s -> NULL (%s)" % (entry, amd_last_error())

    def __enter__(self): return self

    def __exit__(self, *a):
        self.L.cfhd_amd_batch_destroy(self.b); self.b = None

    def upload(self, frames, row):
        for i, f in enumerate(frames):
            f = np.ascontiguousarray(f)
            assert self.L.cfhd_amd_batch_upload(self.b, i, f.ctypes.data_as(V), row) == 0, amd_last_error()

    def frame(self, i, row):
        out = np.full((self.h, row), 0x5a, np.uint8)
        rc = self.L.cfhd_amd_batch_download_frame(self.b, i, out.ctypes.data_as(V), row)
        assert rc == 0, (rc, amd_last_error())
        return out

    def run(self):
        total = self.L.cfhd_amd_batch_roundtrip(self.b)
        assert total > 0, (total, amd_last_error())
        return DP.batch_samples(self.L, self.b, self.n)

    def outputs(self, row):
        out = []
        for i in range(self.n):
            o = np.full((self.h, row), 0x5a, np.uint8)
            assert self.L.cfhd_amd_batch_download_output(self.b, i, o.ctypes.data_as(V), row) == 0, amd_last_error()
            out.append(o)
        return out


RG48_444 = ("ex", PIX_RG48, ENCODED_RGB444, 0, QUALITY_FILMSCAN1)


def compare_frame(got, want, what):
    if np.array_equal(got, want): return
    g, w = got.view(np.uint16).reshape(-1), want.view(np.uint16).reshape(-1)
    bad = np.flatnonzero(g != w)
    raise AssertionError("%s: %d of %d words differ, first at word %d: %d, expected %d" % (what, bad.size, g.size, int(bad[0]), int(g[bad[0]]), int(w[bad[0]])))


# ---- 1. the word rule, whole
RULE_W = RULE_H = 256


def all_patterns_planes():
    """One frame's three planes of 16-bit patterns, all 65 536 in each: identity, reversed, i * 40503 mod 65536.  uint8 [3, 256, 512]."""
    i = np.arange(65536, dtype=np.uint32)
    planes = np.stack([i, 65535 - i, (i * 40503) & 0xffff]).astype(np.uint16)
    assert all(np.unique(p).size == 65536 for p in planes)
    return np.ascontiguousarray(planes).view(np.uint8).reshape(3, RULE_H, RULE_W * 2)


_f32_set = []


def f32_rule_values():
    """The float32 values of test 1, as many as two frames hold (6 x 65 536): for every k in 0 .. 65534 the single nearest (k + 0.5) / 65535 and its two neighbours --
    after the one single multiply, 65 537 of those products are exact ties, 32 768 of them on an even floor --, the specials, random 32-bit patterns for the rest."""
    if _f32_set: return _f32_set[0]
    k = np.arange(65535, dtype=np.float64)
    c = ((k + 0.5) / 65535.0).astype(np.float32)
    near = np.stack([np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))], axis=1).reshape(-1)
    assert near.dtype == np.float32 and near.size == 196605
    prod = (near * np.float32(65535)).astype(np.float64)
    ties = prod[(prod - np.floor(prod)) == 0.5]
    print("%d exact ties among the %d products, %d on an even floor" % (ties.size, near.size, int((np.floor(ties) % 2 == 0).sum())))
    assert ties.size == 65537 and int((np.floor(ties) % 2 == 0).sum()) == 32768      # (what the test rests on: a round-half-up or a double multiply misses these)
    specials = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff], np.uint32).view(np.float32)
    more = np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), np.float32(1e-45), -1e30, 1e30], np.float32)
    assert more[2].view(np.uint32) == 1
    rest = np.random.default_rng(20).integers(0, 1 << 32, 6 * 65536 - near.size - specials.size - more.size, dtype=np.uint64).astype(np.uint32).view(np.float32)
    values = np.concatenate([near, specials, more, rest])
    values.setflags(write=False)
    _f32_set.append(values)
    return values


def check_word_rule(layout):
    w, h = RULE_W, RULE_H
    if layout == PLANAR_F32: frames = list(np.ascontiguousarray(f32_rule_values()).view(np.uint8).reshape(2, 3, h, w * 4))
    else: frames = [all_patterns_planes()]
    n = len(frames)
    with Batch(RG48_444, w, h, n) as bt:
        src = Source(frames, w, h, layout, False)
        assert src.pitch == w * ELEMENT[layout] and src.stride == 3 * h * src.pitch
        src.feed(bt.L, bt.b, 0, n)
        for i in range(n):
            want = expected_words(frames[i], layout)
            if layout == PLANAR_F16:
                largest_subnormal = int(np.flatnonzero(frames[i].view(np.uint16).reshape(-1) == 0x03ff)[0])
                assert want.reshape(-1)[largest_subnormal] == 4, "the largest binary16 subnormal, 1023 x 2^-24: 3.996 of a word"
            compare_frame(bt.frame(i, 6 * w), packed_frame(want), "%s, frame %d" % (LAYOUT_NAMES[layout], i))
        src.unchanged(LAYOUT_NAMES[layout])


def check_delivery_is_inverted(layout):
    """collect(deliver(w)) = w for all 65 536 words: a picture through device_pictures.planar_bytes (numpy's statement of the delivery rules), fed, comes back as it was."""
    assert layout in (PLANAR_U16, PLANAR_F32)
    w, h = RULE_W, RULE_H
    picture = packed_frame(all_patterns_planes().view(np.uint16).reshape(3, h, w))
    planes = planes_of(picture, w, h, layout)
    with Batch(RG48_444, w, h, 1) as bt:
        src = Source([planes], w, h, layout, False)
        src.feed(bt.L, bt.b, 0, 1)
        compare_frame(bt.frame(0, 6 * w), picture, "%s of the delivered picture" % LAYOUT_NAMES[layout])


# ---- 2. geometry, and nothing else touched
GEOMETRY_SHAPES = [(192, 96), (528, 64)]      # 24 lanes a row (a partial wave); 66 lanes (a row crosses a wave)


def geometry_frames(w, h, layout):
    """Four frames of elements whose words differ everywhere: the random RG48 frames by the delivery rules (f16 loses bits; the rule is applied to what is fed)."""
    import gop_input_frames
    frames, row = gop_input_frames.frames("RG48", w, h, 4)
    assert row == 6 * w
    return [planes_of(f, w, h, layout) for f in frames]


def check_geometry(w, h, layout):
    frames = geometry_frames(w, h, layout)
    want = [packed_frame(expected_words(f, layout)) for f in frames]
    assert len(set(x.tobytes() for x in want)) == 4
    for padded in (False, True):
        what = "%dx%d, %s, %s" % (w, h, LAYOUT_NAMES[layout], "pitch with padding" if padded else "contiguous tensor")
        src = Source(frames, w, h, layout, padded)
        if padded: assert src.pitch == ((src.row + 15) & ~15) + 48 and src.stride == 3 * h * src.pitch + 4096
        else: assert src.pitch == src.row and src.stride == 3 * h * src.row
        with Batch(RG48_444, w, h, 4) as bt:
            for first, count in ((1, 2), (0, 1), (3, 1)): src.feed(bt.L, bt.b, first, count)
            for i in range(4): compare_frame(bt.frame(i, 6 * w), want[i], "%s, frame %d" % (what, i))
        # frames 1 - 2 alone, over frames cfhd_amd_batch_upload put there
        held = [np.ascontiguousarray(want[(i + 2) % 4][::-1]) for i in range(4)]
        with Batch(RG48_444, w, h, 4) as bt:
            bt.upload(held, 6 * w)
            src.feed(bt.L, bt.b, 1, 2)
            for i in range(4): compare_frame(bt.frame(i, 6 * w), want[i] if i in (1, 2) else held[i], "%s, frames 1 - 2 over uploaded frames, frame %d" % (what, i))
        src.unchanged(what)


# ---- 3. every kind of batch
# (create_stream at HIGH: at 192 x 96 the bit-rate limiter behind that word never engages -- cfhd_amd_quantizer_is_static answers 1 --, so the tables of that stream
# stand still; the two FILMSCAN2 streams are the ones whose tables move, with windows of the batch coded again behind round 0)
KINDS = {"intra-422": ("ex", PIX_RG48, ENCODED_YUV422, 0, QUALITY_FILMSCAN1), "intra-444": RG48_444,
         "groups": ("groups", PIX_RG48, 0, 0, QUALITY_FILMSCAN1), "stream-high": ("stream", PIX_RG48, ENCODED_YUV422, 0, HIGH),
         "group-stream": ("group_stream", PIX_RG48, 0, 0, QUALITY_FILMSCAN1),
         "stream-filmscan2": ("stream", PIX_RG48, ENCODED_YUV422, 0, FILMSCAN2), "group-stream-filmscan2": ("group_stream", PIX_RG48, 0, 0, FILMSCAN2)}
MOVING = {"stream-filmscan2": (ENCODED_YUV422, 0), "group-stream-filmscan2": (0, ENCODING_FLAGS_2FRAME_GOP)}
KIND_CASES = [(k, 1) for k in KINDS] + [("intra-444", 0)]
KIND_IDS = ["%s-mode%d" % c for c in KIND_CASES]
_host_fed = {}


def host_fed(kind, mode, w, h, frames):
    key = (kind, mode, w, h, bool(use_emulated()))
    if key not in _host_fed:
        with Batch(KINDS[kind], w, h, 4, mode) as bt:
            bt.upload(frames, 6 * w)
            samples = bt.run()
            _host_fed[key] = (samples, bt.outputs(6 * w) if mode == 0 else None)
    return _host_fed[key]


def check_kind(kind, mode, layout):
    import gop_input_frames
    w, h = 192, 96
    assert layout in (PLANAR_U16, PLANAR_F32)
    frames, row = gop_input_frames.frames("RG48", w, h, 4)
    frames = [np.asarray(f).reshape(h, row) for f in frames]
    if kind in MOVING: assert lib().cfhd_amd_quantizer_is_static(w, h, PIX_RG48, MOVING[kind][0], MOVING[kind][1], FILMSCAN2) == 0, "the tables of this stream move"
    first, first_out = host_fed(kind, mode, w, h, frames)
    assert len(set(first)) == 4 or "group" in kind      # (groups: two group samples, two 24-byte P-frame samples)
    src = Source([planes_of(f, w, h, layout) for f in frames], w, h, layout, True)
    with Batch(KINDS[kind], w, h, 4, mode) as bt:
        src.feed(bt.L, bt.b, 0, 4)
        second = bt.run()
        if kind in MOVING:
            stats = (ctypes.c_int * 3)()
            assert bt.L.cfhd_amd_batch_stream_stats(bt.b, stats) == 0
            print("%s: %d rounds, %d frames coded, %d units whose tables moved" % (kind, stats[0], stats[1], stats[2]))
        for i in range(4): assert second[i] == first[i], "%s, %s: sample %d of the batch fed planar differs (%d / %d bytes)" % (kind, LAYOUT_NAMES[layout], i, len(second[i]), len(first[i]))
        if mode == 0:
            for i, o in enumerate(bt.outputs(6 * w)): assert np.array_equal(o, first_out[i]), "%s, %s: picture %d of the batch fed planar differs" % (kind, LAYOUT_NAMES[layout], i)
        for i in range(4): compare_frame(bt.frame(i, 6 * w), frames[i], "%s: frame %d behind the pass" % (kind, i))
    src.unchanged(kind)


def check_chunks():
    """An intra batch cut into chunks with streams of their own (CFHD_AMD_CHUNK=3: frames 0 - 2 | 3): a run that crosses the cut is split per chunk."""
    import gop_input_frames
    w, h = 192, 96
    frames, row = gop_input_frames.frames("RG48", w, h, 4)
    frames = [np.asarray(f).reshape(h, row) for f in frames]
    first, _ = host_fed("intra-444", 1, w, h, frames)
    src = Source([planes_of(f, w, h, PLANAR_F32) for f in frames], w, h, PLANAR_F32, True)
    before = os.environ.get("CFHD_AMD_CHUNK")
    os.environ["CFHD_AMD_CHUNK"] = "3"
    try:
        with Batch(RG48_444, w, h, 4) as bt:
            src.feed(bt.L, bt.b, 1, 3); src.feed(bt.L, bt.b, 0, 1)
            for i in range(4): compare_frame(bt.frame(i, 6 * w), frames[i], "chunks of 3 and 1, frame %d" % i)
            second = bt.run()
            for i in range(4): assert second[i] == first[i], "chunks of 3 and 1: sample %d differs" % i
    finally:
        if before is None: del os.environ["CFHD_AMD_CHUNK"]
        else: os.environ["CFHD_AMD_CHUNK"] = before
    src.unchanged("chunks")


# ---- 4. the chain, all in HBM: decode queue -> planar pictures -> frame queue
def check_chain(layout):
    w, h = 192, 96
    samples = DQ.samples_of("422", w, h, DP.source())
    want, geo = DP.case_want("422", w, h, "RG48", DQ.FULL)
    q = DQ.Queue(samples[0], "RG48", DQ.FULL, 8)
    try:
        assert geo == (q.w, q.h, q.row_bytes) and q.row_bytes == 6 * w
        d = DP.Delivery(q, layout, True, 8); d.set()
        ret, status = DP.run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        def device_feed(L, b):
            lib()
            assert L.cfhd_amd_batch_upload_device_planar(b, 0, 8, d.mem.ptr + GUARD, d.stride, d.pitch, layout) == 0, amd_last_error()
        chained = encode_batch(PIX_RG48, ENCODED_RGB444, 0, w, h, 8, device_feed)
    finally:
        q.close()
    # u16, f32: the handle's pictures themselves; f16: what the rule makes of their binary16 elements
    if layout == PLANAR_F16: frames = [packed_frame(expected_words(planes_of(p, w, h, layout), layout)) for p in want]
    else: frames = [np.asarray(p).reshape(h, 6 * w) for p in want]
    def host_feed(L, b):
        for i in range(8): assert L.cfhd_amd_batch_upload(b, i, np.ascontiguousarray(frames[i]).ctypes.data_as(V), 6 * w) == 0
    direct = encode_batch(PIX_RG48, ENCODED_RGB444, 0, w, h, 8, host_feed)
    assert len(set(direct)) == 8
    for i in range(8): assert chained[i] == direct[i], "%s: sample %d of the chain differs from the sample of the frame uploaded from the host" % (LAYOUT_NAMES[layout], i)


# ---- 5. gates
def check_gates():
    w, h = 192, 96
    L = lib()
    frames = geometry_frames(w, h, PLANAR_F32)
    src = Source(frames, w, h, PLANAR_F32, True)
    p, stride, pitch = src.at(0), src.stride, src.pitch
    def refused(b, first, count, ptr, s, pt, layout, what):
        assert L.cfhd_amd_batch_upload_device_planar(b, first, count, ptr, s, pt, layout) == -1, what
        text = amd_last_error()
        assert text and "planar" in text, "%s: refused without a text (%r)" % (what, text)
        return text
    refused(None, 0, 1, p, stride, pitch, PLANAR_F32, "no batch")
    with Batch(("ex", PIX_YUY2, ENCODED_YUV422, 0, QUALITY_FILMSCAN1), w, h, 4) as yuy2:
        assert "RG48" in refused(yuy2.b, 0, 1, p, stride, pitch, PLANAR_U16, "a YUY2 batch")
    with Batch(RG48_444, w, h, 4) as bt:
        b = bt.b
        texts = [refused(b, 0, 1, p, stride, pitch, 0, "layout 0 (packed)"), refused(b, 0, 1, p, stride, pitch, 4, "an unknown layout"), refused(b, 0, 1, p, stride, pitch, -1, "a negative layout"),
                 refused(b, 0, 0, p, stride, pitch, PLANAR_F32, "count 0"), refused(b, 0, -1, p, stride, pitch, PLANAR_F32, "a negative count"),
                 refused(b, -1, 1, p, stride, pitch, PLANAR_F32, "a run that starts in front of the batch"), refused(b, 3, 2, p, stride, pitch, PLANAR_F32, "a run that leaves the batch"),
                 refused(b, 4, 1, p, stride, pitch, PLANAR_F32, "a run behind the batch"), refused(b, 0, 5, p, stride, pitch, PLANAR_F32, "more frames than the batch holds"),
                 refused(b, 0, 1, None, stride, pitch, PLANAR_F32, "no pointer"),
                 refused(b, 0, 1, p + 8, stride, pitch, PLANAR_F32, "a pointer off 16"), refused(b, 0, 2, p, stride + 8, pitch, PLANAR_F32, "a stride off 16"),
                 refused(b, 0, 1, p, stride, pitch + 8, PLANAR_F32, "a pitch off 16"),
                 refused(b, 0, 1, p, stride, -pitch, PLANAR_F32, "a negative pitch"), refused(b, 0, 1, p, stride, w * 4 - 16, PLANAR_F32, "a pitch below the f32 row bytes"),
                 refused(b, 0, 1, p, stride, w * 2 - 16, PLANAR_U16, "a pitch below the u16 row bytes"), refused(b, 0, 1, p, stride, w * 2 - 16, PLANAR_F16, "a pitch below the f16 row bytes"),
                 refused(b, 0, 2, p, 3 * h * pitch - 16, pitch, PLANAR_F32, "a stride below three planes")]
        assert len(set(texts)) >= 6, texts
        # nothing was launched: the frames are what upload put there
        held = [packed_frame(expected_words(f, PLANAR_F32))[::-1].copy() for f in frames]
        bt.upload(held, 6 * w)
        refused(b, 0, 1, p, stride, w * 4 - 16, PLANAR_F32, "a pitch below the f32 row bytes, again")
        for i in range(4): compare_frame(bt.frame(i, 6 * w), held[i], "behind refused calls, frame %d" % i)
        # the smallest pitch and stride are served
        tight = Source(frames, w, h, PLANAR_F32, False)
        assert L.cfhd_amd_batch_upload_device_planar(b, 0, 4, tight.at(0), 3 * h * w * 4, w * 4, PLANAR_F32) == 0, amd_last_error()
        # a pass in flight refuses both entry points, bad arguments refuse download_frame
        out = np.zeros((h, 6 * w), np.uint8)
        assert L.cfhd_amd_batch_download_frame(b, 4, out.ctypes.data_as(V), 6 * w) == -1 and L.cfhd_amd_batch_download_frame(b, -1, out.ctypes.data_as(V), 6 * w) == -1
        assert L.cfhd_amd_batch_download_frame(b, 0, None, 6 * w) == -1 and L.cfhd_amd_batch_download_frame(b, 0, out.ctypes.data_as(V), 6 * w - 2) == -1
        assert L.cfhd_amd_batch_download_frame(None, 0, out.ctypes.data_as(V), 6 * w) == -1
        assert L.cfhd_amd_batch_submit(b) == 0, amd_last_error()
        try:
            assert "flight" in refused(b, 0, 1, p, stride, pitch, PLANAR_F32, "a pass in flight")
            assert L.cfhd_amd_batch_download_frame(b, 0, out.ctypes.data_as(V), 6 * w) == -1, "download_frame with a pass in flight"
        finally:
            total = L.cfhd_amd_batch_wait(b)
        assert total > 0, (total, amd_last_error())
        want = [packed_frame(expected_words(f, PLANAR_F32)) for f in frames]
        for i in range(4): compare_frame(bt.frame(i, 6 * w), want[i], "behind the pass, frame %d" % i)
    src.unchanged("gates")


def check_download_frame_of_other_inputs():
    """cfhd_amd_batch_download_frame serves every kind of batch and input format: a YUY2 intra batch and a YUY2 batch of groups give back what upload put there, at a
    pitch wider than the rows."""
    w, h = 192, 96
    frames = [np.ascontiguousarray(DQ._yuy2_frame(w, h, i, False)).view(np.uint8).reshape(h, 2 * w) for i in range(4)]
    for kind in (("ex", PIX_YUY2, ENCODED_YUV422, 0, QUALITY_FILMSCAN1), ("groups", PIX_YUY2, 0, 0, QUALITY_FILMSCAN1)):
        with Batch(kind, w, h, 4) as bt:
            bt.upload(frames, 2 * w)
            for i in range(4):
                got = bt.frame(i, 2 * w + 32)
                assert np.array_equal(got[:, : 2 * w], frames[i]) and (got[:, 2 * w:] == 0x5a).all(), "%s: frame %d" % (kind[0], i)


# ---- 7. the host statement of the rule
RULE_PROGRAM = r"""
// the element rules of cfhd_collect_kernels.h as a host compiler builds them: "h <binary16 pattern> <word>" for all 65 536 patterns, then "f <single's bits> <word>"
// for every 32-bit pattern of the file named on the command line
#include "hip_emu.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
#include "cfhd_collect_kernels.h"
#include <stdio.h>
#include <vector>
int main(int argc, char **argv)
{
	for (unsigned h = 0; h < 65536u; h++) printf("h %u %u\n", h, cfhd::dev::collect_word_f16(h));
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 3;
	std::vector<unsigned> bits(1 << 16);
	for (size_t n; (n = fread(bits.data(), 4, bits.size(), f)) > 0;)
		for (size_t k = 0; k < n; k++) { float x; memcpy(&x, &bits[k], 4); printf("f %u %u\n", bits[k], cfhd::dev::collect_word_f32(x)); }
	fclose(f);
	return 0;
}
"""


def check_host_statement():
    """All binary16 patterns and the float32 set of check_word_rule through the host-compiled conversion functions, against numpy."""
    build = os.path.join(ROOT, "tests", "_build"); os.makedirs(build, exist_ok=True)
    src, exe, data = os.path.join(build, "collect_words.cpp"), os.path.join(build, "collect_words"), os.path.join(build, "collect_words_f32.bin")
    header = os.path.join(PRODUCT_DIR, "csrc", "cfhd_collect_kernels.h")
    if not os.path.exists(src) or open(src).read() != RULE_PROGRAM: open(src, "w").write(RULE_PROGRAM)
    DP.cfhd_testlib_build_once(exe, ["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hipemu"), "-I" + os.path.join(PRODUCT_DIR, "csrc"), src], [src, header])
    values = f32_rule_values()
    values.view(np.uint32).tofile(data)
    lines = subprocess.run([exe, data], capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    half = np.array([[int(x) for x in line.split()[1:]] for line in lines if line.startswith("h ")], dtype=np.uint32)
    assert half.shape == (65536, 2) and np.array_equal(half[:, 0], np.arange(65536))
    want = expected_words(np.arange(65536, dtype=np.uint16).view(np.uint8), PLANAR_F16)
    bad = np.flatnonzero(half[:, 1] != want)
    assert bad.size == 0, "%d binary16 patterns differ from numpy, first %#x: %d, numpy %d" % (bad.size, int(bad[0]), int(half[bad[0], 1]), int(want[bad[0]]))
    assert want[0x03ff] == 4 and want[0x0001] == 0 and want[0x3c00] == 65535 and want[0x7e00] == 0 and want[0xfc00] == 0 and want[0x7c00] == 65535
    single = np.array([[int(x) for x in line.split()[1:]] for line in lines if line.startswith("f ")], dtype=np.uint32)
    assert single.shape == (values.size, 2) and np.array_equal(single[:, 0], values.view(np.uint32))
    want = expected_words(np.ascontiguousarray(values).view(np.uint8), PLANAR_F32)
    bad = np.flatnonzero(single[:, 1] != want)
    assert bad.size == 0, "%d singles differ from numpy, first bits %#x: %d, numpy %d" % (bad.size, int(single[bad[0], 0]), int(single[bad[0], 1]), int(want[bad[0]]))


# ---- 8. the kernel's time (hardware)
def check_kernel_time():
    w, h = 192, 96
    L = lib()
    frames = geometry_frames(w, h, PLANAR_F32)
    src = Source(frames, w, h, PLANAR_F32, False)
    packed = [packed_frame(expected_words(f, PLANAR_F32)) for f in frames]
    image = np.concatenate([x.reshape(-1) for x in packed])
    mem = DeviceArray(image)
    with Batch(RG48_444, w, h, 4) as bt:
        assert L.cfhd_amd_batch_kernel_name(bt.b, 20) == b"k_enc_collect"
        src.feed(bt.L, bt.b, 0, 2); src.feed(bt.L, bt.b, 2, 2)
        first = bt.run()
        ms = L.cfhd_amd_batch_kernel_ms(bt.b, 20)
        print("k_enc_collect, two launches of two frames: %.4f ms" % ms)
        assert ms > 0 and L.cfhd_amd_batch_kernel_name(bt.b, 20) == b"k_enc_collect", ms
        for i in range(4): assert L.cfhd_amd_batch_upload_device(bt.b, i, mem.ptr + i * 6 * w * h, 6 * w) == 0, amd_last_error()
        bt.run()
        assert L.cfhd_amd_batch_kernel_ms(bt.b, 20) == 0, "a pass fed by upload_device has no collect time"
        assert len(set(first)) == 4
