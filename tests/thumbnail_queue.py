"""Thumbnail batches of the decode queue (cfhd_amd_decode_batch_create_thumbnails: the 1/8 x 1/8 DPX0 picture of every sample of a pass from its raw lowpass words,
k_dec_thumbnail; delivered packed or as R, G, B planes of the 10-bit values, k_dec_deliver_rgb10): the helpers and test bodies shared by
tests/test_gpu_thumbnail_queue.py (hardware) and tests/test_thumbnail_queue_emulated.py (the same functions inside cfhd_testlib.emulated_product()).

The witnesses: the product's own CFHD_GetThumbnail on each sample -- host code, pinned byte for byte on the reference by tests/test_host_bitstream.py --, the
reference's CFHD_GetThumbnail where oracle/_ref is built, and for the planes numpy's unpacking of the packed words w (big-endian longwords): r = w >> 22,
g = (w >> 12) & 1023, b = (w >> 2) & 1023; u16 the value, f32 value.astype(float32) * (float32(1) / float32(1023)), f16 that .astype(float16), compared as bit
patterns.  Everything is byte for byte: no tolerance anywhere.  A device buffer is checked whole (device_pictures.Delivery: pattern, guards, every byte of padding).
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import device_pictures as DP
from decode_queue import pack, scattered_blob, device_copy, damaged, use_emulated, V, _sizes
from device_pictures import GUARD, pattern, DeviceArray

PACKED, RGB10_U16, RGB10_F16, RGB10_F32 = 0, 19, 20, 21
LAYOUTS = (PACKED, RGB10_U16, RGB10_F16, RGB10_F32)
LAYOUT_NAMES = {PACKED: "packed", RGB10_U16: "u16", RGB10_F16: "f16", RGB10_F32: "f32"}
ELEMENT = {RGB10_U16: 2, RGB10_F16: 2, RGB10_F32: 4}
OKAY, BADSAMPLE = 0, 5
ZERO = "zero"
# (kind of sample, width, height): 24 x 12 -- W8 a multiple of 8 --, the same interlaced, 26 x 13 -- chroma rows of 13 words, every second one off a longword boundary;
# luma rows off 16-byte boundaries; 338 pixels, no multiple of 8; every second picture off a 16-byte boundary --, the RGB families at 24 x 12 and 22 x 13, RGBA (the
# fourth channel ignored)
GEOMETRIES = [("422", 192, 96), ("422i", 192, 96), ("422", 208, 104), ("444", 192, 96), ("444", 176, 104), ("4444", 192, 96)]
GEOMETRY_IDS = ["%s-%dx%d" % g for g in GEOMETRIES]
# more pixels in the picture (528 x 12 = 6336) than one workgroup of k_dec_thumbnail covers in one step (256 lanes x 8 pixels = 2048; the grid has two pieces, so every
# workgroup takes two steps), and a thumbnail row (528 pixels) longer than one wave's step of k_dec_deliver_rgb10 (64 lanes x 8 pixels = 512)
BIG = ("422", 4224, 96)

TEXT_LAYOUT = "decode queue: a thumbnail batch delivers its DPX0 words (CFHD_AMD_PICTURES_PACKED) or the planes R, G, B of their 10-bit values (CFHD_AMD_PICTURES_RGB10_U16 / _F16 / _F32)"
TEXT_UNKNOWN = "decode queue: unknown layout of the device pictures"
TEXT_OFF_16 = "decode queue: the device pictures' pointer, stride and pitch are multiples of 16"
TEXT_LOW_PITCH = "decode queue: the pitch is below the plane row of the RGB10 layout (width x element size)"
TEXT_LOW_STRIDE = "decode queue: the stride is below the three planes of the RGB10 layout (3 x H rows a pitch apart)"
TEXT_PACKED_LOW_PITCH = "decode queue: the device pictures' pitch is below the row bytes of the layout"
TEXT_PACKED_LOW_STRIDE = "decode queue: the device pictures' stride is below what one picture occupies"


def source():
    """The reference's samples where oracle/_ref is built, the product's otherwise."""
    return "ref" if have_ref() else "amd"


def lib():
    L = DP.lib()
    if not getattr(L, "_thumbnail_queue_declared", False):
        L.cfhd_amd_decode_batch_create_thumbnails.restype = V
        L.cfhd_amd_decode_batch_create_thumbnails.argtypes = [V, ctypes.c_size_t, ctypes.c_int]
        L._thumbnail_queue_declared = True
    return L


_THUMB_ARGS = [V, V, ctypes.c_size_t, V, ctypes.c_size_t, ctypes.c_uint32] + [ctypes.POINTER(ctypes.c_size_t)] * 3


def get_thumbnail(L, sample, size=None):
    """(return code, w, h, the bytes) of CFHD_GetThumbnail of library L on a handle of its own, into a buffer no thumbnail here outgrows."""
    dec = V(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        sb = ctypes.create_string_buffer(sample, len(sample)); out = np.zeros(1024 * 64 * 4, np.uint8)
        w = ctypes.c_size_t(); h = ctypes.c_size_t(); n = ctypes.c_size_t()
        L.CFHD_GetThumbnail.argtypes = _THUMB_ARGS
        rc = L.CFHD_GetThumbnail(dec, sb, len(sample) if size is None else size, out.ctypes.data_as(V), out.size, 0, ctypes.byref(w), ctypes.byref(h), ctypes.byref(n))
        return rc, w.value, h.value, out[: n.value].copy() if rc == 0 else None
    finally:
        L.CFHD_CloseDecoder(dec)


def witness(sample, size=None): return get_thumbnail(product(), sample, size)


def expected(sample, size, w8, h8):
    """(status, picture) a batch of w8 x h8 thumbnails owes this sample: CFHD_GetThumbnail's answer; BADSAMPLE for a thumbnail of another geometry; zeros for a failure."""
    rc, w, h, picture = witness(sample, size)
    if rc == 0 and (w, h) != (w8, h8): rc = BADSAMPLE
    return rc, picture if rc == 0 else np.zeros(4 * w8 * h8, np.uint8)


# ---- frames and samples
# (Y, U, V) of the 4:2:2 patches and (R, G, B) of the RGB ones: white, black and the six corners between them.  Through the thumbnail's matrix every one of r, g, b
# runs into both clamps on them (1192 x 956 + 1836 x 508 >> 10 = 2023; 1192 x -64 - 1836 x 512 < 0; ...)
CORNERS = ((1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1))


def _yuy2_frames(w, h, n, interlaced):
    """n distinct textured frames with a band of patches 16 pixels wide and 16 rows high across the top -- the lowpass band is the 8 x 8 block mean: two whole lowpass
    pixels a side -- , luma 0 or 255 against chroma 0 or 255, plus white and black with neutral chroma; the band moves by a patch from frame to frame."""
    patches = [tuple(255 * c for c in p) for p in CORNERS] + [(255, 128, 128), (0, 128, 128)]
    out = []
    for i in range(n):
        f = np.array(DQ._yuy2_frame(w, h, i, interlaced)).reshape(h, w // 2, 4)
        for k in range(w // 16):
            y, u, v = patches[(k + i) % len(patches)]
            f[:16, 8 * k: 8 * k + 8] = (y, u, y, v)
        out.append(np.ascontiguousarray(f).reshape(-1))
    return out


def _rgb_frames(fmt, w, h, n):
    import gop_input_frames
    frames, pitch = gop_input_frames.frames(fmt, w, h, n)
    words = 3 if fmt == "RG48" else 4
    out = []
    for i, f in enumerate(frames):
        px = np.array(f).view(np.uint16).reshape(h, w, words)
        for k in range(w // 16): px[:16, 16 * k: 16 * k + 16, words - 3:] = [65535 * c for c in CORNERS[(k + i) % 8]]
        out.append(np.ascontiguousarray(px).view(np.uint8).reshape(-1))
    return out, pitch


def walk_lowpass(sample):
    """[(position of the size chunk, position of the first lowpass word, width, height)] of every channel's raw lowpass band, by the tag walk of parse_sample."""
    d = sample; pos = 0; pending_at = pending = chunk_pos = lw = lh = 0; out = []
    while pos + 4 <= len(d):
        tag = int.from_bytes(d[pos: pos + 2], "big", signed=True); value = int.from_bytes(d[pos + 2: pos + 4], "big")
        tag = -tag if tag < 0 else tag
        here = pos; pos += 4
        if tag & 0x4000:
            pos += 4 * ((((tag & 0xff) << 16) | value) if tag & 0x2000 else value); continue
        if tag & 0x2000:
            if (tag & 0xff00) == 0x2000: pending = 4 * (((tag & 0xff) << 16) | value); pending_at = pos; chunk_pos = here
            continue
        if tag == 2: pos += 4 * value
        elif tag == 27: lw = value
        elif tag == 28: lh = value
        elif tag == 4 and value == 0x0f0f: out.append((chunk_pos, pos, lw, lh)); pos = pending_at + pending
        elif tag == 55: pos = pending_at + pending
    return out


def random_lowpass(sample, seed):
    """The sample with the raw lowpass words of every channel overwritten by seeded random 16-bit words over the whole range: the bits above the ten, the negative side
    of the arithmetic shift."""
    s = bytearray(sample); rng = np.random.default_rng(seed)
    bands = walk_lowpass(sample)
    assert len(bands) >= 3
    for _, at, lw, lh in bands: s[at: at + 2 * lw * lh] = rng.integers(0, 256, 2 * lw * lh, dtype=np.uint8).tobytes()
    return bytes(s)


_samples = {}


def samples_of(kind, w, h, n=8, src=None):
    """n samples of n distinct patched frames, kind "422", "422i", "444" (RG48 -> RGB 4:4:4) or "4444" (b64a -> RGBA 4:4:4:4); the last but two with random lowpass
    words; encoded once, shared, read-only."""
    src = src or source()
    key = (kind, w, h, n, src, bool(use_emulated()))
    if key not in _samples:
        if kind in ("422", "422i"): frames, pitch, pix, enc, flags = _yuy2_frames(w, h, n, kind == "422i"), w * 2, PIX_YUY2, ENCODED_YUV422, int(kind == "422i")
        elif kind == "444": (frames, pitch), pix, enc, flags = _rgb_frames("RG48", w, h, n), PIX_RG48, ENCODED_RGB444, 0
        else: (frames, pitch), pix, enc, flags = _rgb_frames("b64a", w, h, n), PIX_B64A, ENCODED_RGBA4444, 0
        encode = ref_encode_frames if src == "ref" else amd_encode_frames
        samples = list(encode([np.ascontiguousarray(f) for f in frames], pitch, w, h, pix, enc, QUALITY_FILMSCAN1, flags))
        assert len(set(samples)) == n
        at = max(n - 3, 0)
        samples[at] = random_lowpass(samples[at], 17 + w)
        _samples[key] = tuple(samples)
    return list(_samples[key])


_witness = {}


def witnesses(kind, w, h, n=8):
    """The witness pictures of samples_of(...): computed once, read-only; every status 0, the geometry (w + 7) // 8 x (h + 7) // 8; the reference's agree where built."""
    key = (kind, w, h, n, source(), bool(use_emulated()))
    if key not in _witness:
        out = []
        for i, s in enumerate(samples_of(kind, w, h, n)):
            rc, tw, th, p = witness(s)
            assert (rc, tw, th) == (0, (w + 7) // 8, (h + 7) // 8), (kind, w, h, i, rc, tw, th)
            if have_ref():
                rrc, rw, rh, rp = get_thumbnail(ref(), s)
                assert (rrc, rw, rh) == (0, tw, th) and np.array_equal(rp, p), "sample %d: the reference's CFHD_GetThumbnail differs from the product's" % i
            p.setflags(write=False); out.append(p)
        _witness[key] = out
    return _witness[key]


def fields(picture):
    """(r, g, b) of packed DPX0 bytes as uint16 arrays."""
    w = np.ascontiguousarray(picture).view(">u4").astype(np.uint32)
    return (w >> 22).astype(np.uint16), ((w >> 12) & 1023).astype(np.uint16), ((w >> 2) & 1023).astype(np.uint16)


def check_clamps(pictures, what):
    """Each of r, g, b holds 0 and 1023 somewhere in the witness pictures: a frame set that never clamps fails here instead of hiding the clamp."""
    for name, plane in zip("rgb", [np.concatenate(c) for c in zip(*[fields(p) for p in pictures])]):
        assert plane.min() == 0 and plane.max() == 1023, "%s: %s spans %d .. %d in the witness pictures: the clamps are not met" % (what, name, plane.min(), plane.max())


# ---- the queue and the expected contents of a device buffer
class ThumbQueue(DQ.Queue):
    """decode_queue.Queue on a thumbnail batch prepared on `first`."""
    def __init__(self, first, n):
        self.L = lib(); self.n = n
        fb = ctypes.create_string_buffer(first, len(first))
        self.b = self.L.cfhd_amd_decode_batch_create_thumbnails(fb, len(first), n)
        assert self.b, "cfhd_amd_decode_batch_create_thumbnails -> NULL (%s)" % amd_last_error()
        w = ctypes.c_int(); h = ctypes.c_int(); rb = ctypes.c_int()
        assert self.L.cfhd_amd_decode_batch_geometry(self.b, ctypes.byref(w), ctypes.byref(h), ctypes.byref(rb)) == 0
        self.w, self.h, self.row_bytes = w.value, h.value, rb.value


def refused(sample, n, size=None):
    L = lib()
    fb = ctypes.create_string_buffer(sample, len(sample)) if sample is not None else None
    b = L.cfhd_amd_decode_batch_create_thumbnails(fb, (len(sample) if size is None else size) if sample is not None else 0, n)
    if b: L.cfhd_amd_decode_batch_destroy(b); return False
    text = amd_last_error()
    assert text, "refused without a text"
    return text


def elements(values, layout):
    """uint16 values [rows, n] in the element type of the layout: uint8 [rows, n * E]."""
    values = np.ascontiguousarray(values)
    if layout == RGB10_U16: return values.view(np.uint8).reshape(values.shape[0], -1)
    f32 = values.astype(np.float32) * (np.float32(1) / np.float32(1023))
    assert f32.dtype == np.float32
    if layout == RGB10_F32: return np.ascontiguousarray(f32).view(np.uint8).reshape(values.shape[0], -1)
    return np.ascontiguousarray(f32.astype(np.float16)).view(np.uint8).reshape(values.shape[0], -1)


def geometry(w, h, layout, padded):
    """(row bytes, pitch, stride): the contiguous form (the pitch rounded up to 16), or a pitch with 48 bytes of padding and a stride of + 4096."""
    row = 4 * w if layout == PACKED else w * ELEMENT[layout]
    pitch = ((row + 15) & ~15) + (48 if padded else 0)
    return row, pitch, (1 if layout == PACKED else 3) * h * pitch + (4096 if padded else 0)


def place(image, at, w, h, layout, pitch, picture):
    """One picture -- its packed bytes, or ZERO -- at image[at:] in the layout."""
    if picture is ZERO: picture = np.zeros(4 * w * h, np.uint8)
    if layout == PACKED:
        image[at: at + h * pitch].reshape(h, pitch)[:, : 4 * w] = np.asarray(picture).reshape(h, 4 * w)
        return
    for c, plane in enumerate(fields(picture)):
        start = at + c * h * pitch
        image[start: start + h * pitch].reshape(h, pitch)[:, : w * ELEMENT[layout]] = elements(plane.reshape(h, w), layout)


class Delivery(DP.Delivery):
    """device_pictures.Delivery for the pictures of a thumbnail batch in one of the four layouts.  The pictures handed to expect / check are packed bytes, ZERO or None
    (untouched)."""
    def __init__(self, q, layout, padded, npictures):
        self.q, self.layout = q, layout
        self.row, self.pitch, self.stride = geometry(q.w, q.h, layout, padded)
        self.image = pattern(GUARD + npictures * self.stride + GUARD)
        self.mem = DeviceArray(self.image)

    def expect(self, pictures):
        for i, p in enumerate(pictures):
            if p is not None: place(self.image, GUARD + i * self.stride, self.q.w, self.q.h, self.layout, self.pitch, p)
        return self.image


def off(q): assert lib().cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0


def _same(a, b, what):
    assert np.array_equal(a, b), "%s: %d bytes differ from CFHD_GetThumbnail's picture" % (what, int((np.asarray(a) != np.asarray(b)).sum()))


def submit_device(q, dptr, blob, offsets, sizes):
    return q.L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, _sizes(offsets), _sizes(sizes), len(offsets))


# ---- 1. exact pictures, both submit paths, every way out
def check_exact(kind, w, h, layout, n=8):
    samples = samples_of(kind, w, h, n)
    want = witnesses(kind, w, h, n)
    if kind in ("422", "422i"): check_clamps(want, "%s %d x %d" % (kind, w, h))
    q = ThumbQueue(samples[0], n)
    try:
        assert (q.w, q.h, q.row_bytes) == ((w + 7) // 8, (h + 7) // 8, 4 * ((w + 7) // 8))
        frame = q.row_bytes * q.h
        blob, offsets, sizes = scattered_blob(samples)      # (shuffled, junk between them, at odd byte offsets)
        # from host memory: the caller's device memory (padded pitch and stride), host delivery, download_output
        d = Delivery(q, layout, True, n); d.set()
        host = np.full(frame * n, 9, np.uint8)
        assert q.submit(blob, offsets, sizes, host, frame, q.row_bytes) == 0, amd_last_error()
        assert q.wait(n) == (n, [0] * n), amd_last_error()
        for i, p in enumerate(q.pictures(n)):
            _same(p, want[i], "submit_host, download_output(%d)" % i)
            _same(host[i * frame: (i + 1) * frame], want[i], "submit_host, host picture %d" % i)
        d.check(want, "submit_host, %s" % LAYOUT_NAMES[layout])
        # from HBM: the contiguous tensor geometry
        owner, dptr = device_copy(blob)
        if dptr is None: dptr = owner.ptr
        d2 = Delivery(q, layout, False, n); d2.set()
        assert submit_device(q, dptr, blob, offsets, sizes) == 0, amd_last_error()
        assert q.wait(n) == (n, [0] * n), amd_last_error()
        for i, p in enumerate(q.pictures(n)): _same(p, want[i], "submit_device, download_output(%d)" % i)
        d2.check(want, "submit_device, %s" % LAYOUT_NAMES[layout])
        d.check([None] * n, "the first buffer behind a pass that delivers elsewhere")
        del owner
    finally:
        q.close()


def check_geometry_of_a_display_height_that_is_no_multiple_of_8():
    """YU64 192 x 100: geometry equals CFHD_GetThumbnail's answer (24 x 13: the encoded height is 104), and so do the pictures."""
    w, h = 192, 100
    rng = np.random.default_rng(4)
    frames = [np.ascontiguousarray((rng.integers(4096, 60000, (h, w * 2)).astype(np.uint16) & 0xffc0)).view(np.uint8).reshape(-1) for _ in range(2)]
    samples = amd_encode_frames(frames, w * 4, w, h, PIX_YU64, ENCODED_YUV422)
    rc, tw, th, p0 = witness(samples[0])
    assert rc == 0 and (tw, th) == (24, 13), (rc, tw, th)
    q = ThumbQueue(samples[0], 2)
    try:
        assert (q.w, q.h, q.row_bytes) == (tw, th, 4 * tw)
        ret, status, pictures = q.decode(samples)
        assert (ret, status) == (2, [0, 0])
        for i in range(2): _same(pictures[i], witness(samples[i])[3], "192 x 100, picture %d" % i)
    finally:
        q.close()


# ---- 2. a short pass, layouts that switch, delivery off
def check_short_pass_and_switching(kind, w, h, first_layout, second_layout):
    samples = samples_of(kind, w, h)
    want = witnesses(kind, w, h)
    q = ThumbQueue(samples[0], 8)
    try:
        d = Delivery(q, first_layout, True, 8); d.set()
        pitch = q.row_bytes + 32; frame = pitch * q.h + 64
        host = np.full(frame * 8, 0x5a, np.uint8)
        blob, offsets, sizes = pack(samples[:5])
        assert q.submit(blob, offsets, sizes, host, frame, pitch) == 0, amd_last_error()
        assert q.wait(5) == (5, [0] * 5)
        d.check(list(want[:5]) + [None] * 3, "a pass of 5 in a batch of 8")
        for i in range(5):
            img = host[i * frame: i * frame + pitch * q.h].reshape(q.h, pitch)
            _same(img[:, : q.row_bytes].reshape(-1), want[i], "host picture %d" % i)
            assert (img[:, q.row_bytes:] == 0x5a).all() and (host[i * frame + pitch * q.h: (i + 1) * frame] == 0x5a).all(), "host picture %d: bytes behind the rows were written" % i
        assert (host[5 * frame:] == 0x5a).all(), "host pictures behind the count were written"
        # another layout, another buffer: the first one keeps what it held
        d2 = Delivery(q, second_layout, False, 8); d2.set()
        assert DP.run_pass(q, samples[::-1]) == (8, [0] * 8)
        d2.check(list(want[::-1]), "the second layout")
        d.check([None] * 8, "the first buffer behind the switch")
        # NULL switches delivery off
        off(q)
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        d.check([None] * 8, "the first buffer with delivery off"); d2.check([None] * 8, "the second buffer with delivery off")
        for i, p in enumerate(q.pictures(8)): _same(p, want[i], "delivery off, download_output(%d)" % i)
    finally:
        q.close()


# ---- 3. failed samples among intact neighbours
# (CFHD_GetThumbnail reads the lowpass bands and never looks at the last bytes of a sample: handed two bytes less it answers OKAY with the picture, and so does the batch,
# by its slow path -- k_dec_ingest does not place a size that is no multiple of 4)
HOST_MADE = ("size no multiple of 4", "rgb of the same geometry")
FAILED_AT = {"truncated": 1, "size no multiple of 4": 3, "damaged tag": 4, "lowpass size chunk": 5, "other geometry": 6, "rgb of the same geometry": 7, "bayer": 8, "group": 9}


def failed_pass():
    """(samples, sizes) of the pass: 4:2:2 192 x 96 samples with one failure of each kind among them."""
    w, h = 192, 96
    good = samples_of("422", w, h)
    samples = [good[i % 8] for i in range(11)]; sizes = [len(s) for s in samples]
    sizes[1] = 200
    sizes[3] = len(samples[3]) - 2
    samples[4], sizes[4] = damaged("frame width", good[4], None)
    s = bytearray(good[5]); at = walk_lowpass(good[5])[0][0]; s[at: at + 4] = b"\x20\xff\xff\xff"; samples[5] = bytes(s)
    samples[6] = samples_of("422", 208, 104)[0]
    samples[7] = samples_of("444", w, h)[0]
    mosaic = synth_bayer(w, h, 7).reshape(-1).view(np.uint8).copy()
    samples[8] = amd_encode_frames([mosaic], w * 2, w, h, PIX_BYR4, ENCODED_BAYER)[0]
    frames = [synth_yuy2(w, h, 20 + i)[0] for i in range(2)]
    samples[9] = amd_encode_frames(frames, w * 2, w, h, PIX_YUY2, flags=ENCODING_FLAGS_2FRAME_GOP)[1]
    for i in (6, 7, 8, 9): sizes[i] = len(samples[i])
    return samples, sizes


def check_failed_samples(layout, from_device=False):
    samples, sizes = failed_pass()
    w8, h8 = 24, 12
    want = [expected(s, z, w8, h8) for s, z in zip(samples, sizes)]
    status = [rc for rc, _ in want]
    print("the witness answers", status)
    assert [status[i] for i in (0, 2, 10)] == [0, 0, 0] and all(status[FAILED_AT[k]] == 0 for k in HOST_MADE) and status[FAILED_AT["other geometry"]] == BADSAMPLE
    assert witness(samples[6])[:3] == (0, 26, 13)            # (the other geometry: a thumbnail CFHD_GetThumbnail makes, not the batch's)
    assert all(status[i] != 0 for k, i in FAILED_AT.items() if k not in HOST_MADE), status
    q = ThumbQueue(samples[0], 12)
    try:
        frame = q.row_bytes * q.h
        d = Delivery(q, layout, True, 12); d.set()
        blob, offsets, _ = pack(samples)
        host = None
        if from_device:
            owner, dptr = device_copy(blob)
            if dptr is None: dptr = owner.ptr
            assert submit_device(q, dptr, blob, offsets, sizes) == 0, amd_last_error()
        else:
            host = np.full(frame * 12, 9, np.uint8)
            assert q.submit(blob, offsets, sizes, host, frame, q.row_bytes) == 0, amd_last_error()
        ret, got = q.wait(11)
        assert got == status, (got, status)
        assert ret == status.count(0)
        pictures = q.pictures(11)
        for i in range(11):
            _same(pictures[i], want[i][1], "download_output(%d)" % i)
            if host is not None: _same(host[i * frame: (i + 1) * frame], want[i][1], "host picture %d" % i)
            if status[i]: assert not pictures[i].any()
        assert pictures[7].any()                                  # (the host's picture of the RGB sample)
        d.check([p for _, p in want] + [None], "failed samples, %s" % LAYOUT_NAMES[layout])
        # an intact pass on the same batch afterwards
        good = samples_of("422", 192, 96); clean = witnesses("422", 192, 96)
        assert DP.run_pass(q, good) == (8, [0] * 8)
        for i, p in enumerate(q.pictures(8)): _same(p, clean[i], "intact pass behind the failures: picture %d" % i)
    finally:
        q.close()


# ---- 4. gates
def check_gates():
    L = lib()
    w, h = 192, 96
    good = samples_of("422", w, h)
    assert refused(None, 4) == "decode queue: no first sample"
    assert refused(good[0], 0) == "decode queue: nsamples < 1"
    assert "65 535" in refused(good[0], 65536)
    frames = [synth_yuy2(w, h, 20 + i)[0] for i in range(3)]
    stream = amd_encode_frames(frames, w * 2, w, h, PIX_YUY2, flags=ENCODING_FLAGS_2FRAME_GOP)
    assert len(stream[0]) == 40 and len(stream[2]) == 24
    group_text = refused(stream[1], 4)
    assert "two-frame groups" in group_text and refused(stream[0], 4) == group_text and refused(stream[2], 4) == group_text
    mosaic = synth_bayer(w, h, 7).reshape(-1).view(np.uint8).copy()
    bayer = amd_encode_frames([mosaic], w * 2, w, h, PIX_BYR4, ENCODED_BAYER)[0]
    assert "Bayer thumbnails" in refused(bayer, 4)
    raw = bytearray(good[0]); at = DQ.walk_bands(good[0])[0][0]; raw[at: at + 4] = b"\x23\x00\x00\x01"
    assert "UNCOMPRESS" in refused(bytes(raw), 4)
    assert "CFHD_GetThumbnail refuses this sample (CFHD_Error 5)" in refused(good[0], 4, size=200)
    # an odd W8: 400 / 8 = 50 is even, 16 x 15 = 240 pixels give 30, 16 x 13 = 208 give 26, 16 x 11 = 176 give 22: RGB 4:4:4 at 200 (width / 8 = 25; 4:2:2 needs width % 16 = 0)
    import gop_input_frames
    (f200, pitch200) = gop_input_frames.frames("RG48", 200, 64, 1)
    odd = amd_encode_frames([np.ascontiguousarray(f200[0])], pitch200, 200, 64, PIX_RG48, ENCODED_RGB444)[0]
    assert witness(odd)[0] != 0
    assert "25 pixels wide" in refused(odd, 4)
    # set_device_pictures
    q = ThumbQueue(good[0], 4)
    try:
        mem = DeviceArray(pattern(GUARD + 4 * 3 * 12 * 128 + GUARD)); p = mem.ptr + GUARD
        def sets(layout, ptr=p, stride=3 * 12 * 96, pitch=96):
            rc = L.cfhd_amd_decode_batch_set_device_pictures(q.b, ptr, stride, pitch, layout)
            return True if rc == 0 else amd_last_error()
        for layout in range(1, 19): assert sets(layout) == TEXT_LAYOUT, layout
        assert sets(22) == TEXT_UNKNOWN and sets(-1) == TEXT_UNKNOWN
        for layout in (RGB10_U16, RGB10_F16, RGB10_F32):
            row = 24 * ELEMENT[layout]
            assert sets(layout, pitch=row, stride=3 * 12 * row) is True
            assert sets(layout, ptr=p + 8, pitch=row, stride=3 * 12 * row) == TEXT_OFF_16
            assert sets(layout, pitch=row + 8, stride=3 * 12 * (row + 8)) == TEXT_OFF_16
            assert sets(layout, pitch=row, stride=3 * 12 * row + 8) == TEXT_OFF_16
            assert sets(layout, pitch=row - 16, stride=3 * 12 * row) == TEXT_LOW_PITCH
            assert sets(layout, pitch=row, stride=3 * 12 * row - 16) == TEXT_LOW_STRIDE
        assert sets(PACKED, pitch=96, stride=12 * 96) is True
        assert sets(PACKED, ptr=p + 4, pitch=96, stride=12 * 96) == TEXT_OFF_16
        assert sets(PACKED, pitch=80, stride=12 * 96) == TEXT_PACKED_LOW_PITCH
        assert sets(PACKED, pitch=96, stride=11 * 96) == TEXT_PACKED_LOW_STRIDE
        off(q)
    finally:
        q.close()
    # cfhd_amd_decode_batch_create refuses and serves what it did on the same samples
    assert "group" in DQ.refused(stream[1], "YUY2", DQ.FULL, 4) and "Bayer" in DQ.refused(bayer, "BYR4", DQ.FULL, 4) and "uncompressed" in DQ.refused(bytes(raw), "YUY2", DQ.FULL, 4)
    assert "nsamples" in DQ.refused(good[0], "YUY2", DQ.FULL, 0)
    # ... and 19 .. 21 are unknown layouts on an ordinary YUY2 batch and an RG48 batch
    for out in ("YUY2", "RG48"):
        plain = DQ.Queue(good[0], out, DQ.FULL, 2)
        try:
            mem = DeviceArray(pattern(2 * plain.row_bytes * plain.h * 4 + 64))
            for layout in (RGB10_U16, RGB10_F16, RGB10_F32):
                assert L.cfhd_amd_decode_batch_set_device_pictures(plain.b, mem.ptr, plain.row_bytes * plain.h * 4, plain.row_bytes * 2, layout) == -1
                assert amd_last_error() == TEXT_UNKNOWN
            assert L.cfhd_amd_decode_batch_set_device_pictures(plain.b, mem.ptr, plain.row_bytes * plain.h, plain.row_bytes, PACKED) == 0
        finally:
            plain.close()


def gates_under_host_entropy():
    """Child process body (CFHD_AMD_ENTROPY=host is read when the library starts its first encoder)."""
    w, h = 192, 96
    sample = amd_encode_frames([synth_yuy2(w, h, 20)[0]], w * 2, w, h)[0]
    text = refused(sample, 4)
    assert text and "CFHD_AMD_ENTROPY" in text, text
    print("HOST ENTROPY REFUSED")


# ---- 5. kernel names and times
def check_kernel_names(times_positive):
    L = lib()
    samples = samples_of("422", 192, 96)
    q = ThumbQueue(samples[0], 8)
    try:
        def names(): return [L.cfhd_amd_decode_batch_kernel_name(q.b, k).decode() for k in range(11)]
        def ms(): return [L.cfhd_amd_decode_batch_kernel_ms(q.b, k) for k in range(11)]
        want = [""] * 11; want[0], want[1], want[6] = "k_dec_ingest", "k_dec_parse", "k_dec_thumbnail"
        assert names() == want
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        assert names() == want
        t = ms(); print("no delivery:", t)
        assert all(t[k] == 0 for k in range(11) if k not in (0, 1, 6)), t
        if times_positive: assert t[0] > 0 and t[1] > 0 and t[6] > 0, t
        for layout, deliver in ((PACKED, "k_dec_deliver"), (RGB10_F16, "k_dec_deliver_rgb10")):
            d = Delivery(q, layout, False, 8); d.set()
            assert DP.run_pass(q, samples) == (8, [0] * 8)
            want[9] = deliver
            assert names() == want
            t = ms(); print(deliver, t)
            assert all(t[k] == 0 for k in range(11) if k not in (0, 1, 6, 9)), t
            if times_positive: assert t[0] > 0 and t[1] > 0 and t[6] > 0 and t[9] > 0, t
        off(q)
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        want[9] = ""
        assert names() == want and ms()[9] == 0
    finally:
        q.close()


def check_queue_rules():
    """One pass per batch at a time, several batches in flight, destroy on a batch in flight."""
    L = lib()
    sets = [samples_of("422", 192, 96), samples_of("444", 192, 96)]
    want = [witnesses("422", 192, 96), witnesses("444", 192, 96)]
    qs = [ThumbQueue(s[0], 8) for s in sets]
    try:
        packed = [pack(s) for s in sets]
        for q, (blob, offsets, sizes) in zip(qs, packed): assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        q = qs[0]; blob, offsets, sizes = packed[0]; x = ctypes.c_int(); buf = np.zeros(q.row_bytes * q.h, np.uint8)
        assert q.submit(blob, offsets, sizes) == -1
        assert L.cfhd_amd_decode_batch_geometry(q.b, ctypes.byref(x), None, None) == -1
        assert L.cfhd_amd_decode_batch_download_output(q.b, 0, buf.ctypes.data_as(V), q.row_bytes) == -1
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == -1
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 6) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 6) == b""
        for k, q in enumerate(qs):
            assert q.wait(8) == (8, [0] * 8)
            for i, p in enumerate(q.pictures(8)): _same(p, want[k][i], "batch %d sample %d" % (k, i))
        assert L.cfhd_amd_decode_batch_wait(qs[0].b, None) == -1
        blob, offsets, sizes = packed[1]
        assert qs[1].submit(blob, offsets, sizes) == 0
        qs[1].close()
    finally:
        for q in qs: q.close()


# ---- 6. a torch tensor (hardware)
def check_torch(torch):
    """torch.empty((n, 3, H8, W8), float16) handed over as device pictures equals the packed words unpacked."""
    samples = samples_of("422", 192, 96)
    want = witnesses("422", 192, 96)
    q = ThumbQueue(samples[0], 8)
    try:
        t = torch.empty((8, 3, q.h, q.w), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        assert lib().cfhd_amd_decode_batch_set_device_pictures(q.b, t.data_ptr(), 3 * q.h * q.w * 2, q.w * 2, RGB10_F16) == 0, amd_last_error()
        assert DP.run_pass(q, samples) == (8, [0] * 8)
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        for i in range(8):
            for c, plane in enumerate(fields(want[i])):
                assert np.array_equal(np.ascontiguousarray(got[i, c]).view(np.uint8).reshape(q.h, q.w * 2), elements(plane.reshape(q.h, q.w), RGB10_F16)), "picture %d plane %d" % (i, c)
    finally:
        q.close()
