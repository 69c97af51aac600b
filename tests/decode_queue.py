"""The decode queue (cfhd_amd_decode_batch_*: batches of intra samples from any encoder, parsed and decoded on the GPU): the helpers and test bodies shared by
tests/test_gpu_decode_queue.py (hardware) and tests/test_decode_queue_emulated.py (the same functions inside cfhd_testlib.emulated_product()).

The yardstick throughout is ONE CFHD_DecodeSample handle of this library, prepared on the same first sample and fed the same samples in the same order: its return
codes are the queue's statuses, its pictures the queue's -- byte for byte for the outputs without dither, within the one dither step for the 8-bit outputs of 4:2:2
samples at full resolution (the queue's seed follows the pass number, the handle's the call count; the interval is the one test_gpu_parity._check_decode uses: a byte
moves by at most one).  What the handle's pictures are worth is pinned on the oracle and the reference by the suites that were here before.
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *

FOURCCS = {"YUY2": PIX_YUY2, "2vuy": PIX_2VUY, "v210": PIX_V210, "RG48": PIX_RG48, "b64a": PIX_B64A, "YU64": PIX_YU64, "RG24": PIX_RG24, "BGRA": PIX_BGRA, "BGRa": PIX_BGRa,
           "DPX0": fourcc("DPX0"), "r210": fourcc("r210"), "BYR4": PIX_BYR4}
FULL, HALF, QUARTER = 1, 2, 3
V = ctypes.c_void_p
SZ = ctypes.POINTER(ctypes.c_size_t)

# (kind of sample, w, h, output, resolution): the outputs that carry no dither -- every picture equals the handle's byte for byte
EXACT_CASES = [("422", 320, 240, "YU64", FULL), ("422", 192, 96, "v210", FULL), ("422", 208, 104, "RG48", FULL), ("422", 320, 240, "YUY2", HALF), ("422", 192, 96, "b64a", HALF),
               ("422i", 320, 240, "RG48", FULL), ("422i", 192, 96, "YUY2", HALF),
               ("444", 192, 96, "RG48", FULL), ("444", 208, 104, "DPX0", FULL), ("4444", 192, 96, "b64a", FULL)]
# (kind, w, h, dithered output, the exact output of the same samples): full-resolution 8-bit outputs of 4:2:2 samples
DITHER_CASES = [("422", 320, 240, "YUY2", "YU64"), ("422", 208, 104, "BGRA", "YU64"), ("422i", 192, 96, "YUY2", "RG48"), ("422i", 320, 240, "BGRA", "RG48")]
SOURCES = ("ref", "amd")
VERDICT_KINDS = ("cut in half", "frame width", "size chunk", "payload pattern", "other geometry", "two bytes")


def lib():
    L = product()
    if not getattr(L, "_decode_queue_declared", False):
        L.cfhd_amd_decode_batch_create.restype = V
        L.cfhd_amd_decode_batch_create.argtypes = [V, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
        L.cfhd_amd_decode_batch_destroy.restype = None; L.cfhd_amd_decode_batch_destroy.argtypes = [V]
        L.cfhd_amd_decode_batch_geometry.argtypes = [V] + [ctypes.POINTER(ctypes.c_int)] * 3
        L.cfhd_amd_decode_batch_submit_host.argtypes = [V, V, SZ, SZ, ctypes.c_int, V, ctypes.c_size_t, ctypes.c_int]
        L.cfhd_amd_decode_batch_submit_device.argtypes = [V, V, ctypes.c_size_t, SZ, SZ, ctypes.c_int]
        L.cfhd_amd_decode_batch_wait.argtypes = [V, ctypes.POINTER(ctypes.c_int)]
        L.cfhd_amd_decode_batch_download_output.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_decode_batch_kernel_ms.restype = ctypes.c_float; L.cfhd_amd_decode_batch_kernel_ms.argtypes = [V, ctypes.c_int]
        L.cfhd_amd_decode_batch_kernel_name.restype = ctypes.c_char_p; L.cfhd_amd_decode_batch_kernel_name.argtypes = [V, ctypes.c_int]
        L.cfhd_amd_register_host_buffer.argtypes = [V, ctypes.c_size_t]; L.cfhd_amd_unregister_host_buffer.argtypes = [V]
        L._decode_queue_declared = True
    return L


def _sizes(values):
    return (ctypes.c_size_t * len(values))(*values)


def pack(samples, sizes=None):
    """The samples back to back in one blob: (blob, offsets, sizes)."""
    sizes = list(sizes) if sizes is not None else [len(s) for s in samples]
    offsets = list(np.cumsum([0] + [len(s) for s in samples[:-1]]))
    return np.frombuffer(b"".join(samples) + b"\0" * 16, np.uint8).copy(), [int(o) for o in offsets], sizes


class Queue:
    """One decode batch prepared on `first`."""
    def __init__(self, first, out, resolution, n):
        self.L = lib(); self.n = n
        fb = ctypes.create_string_buffer(first, len(first))
        self.b = self.L.cfhd_amd_decode_batch_create(fb, len(first), FOURCCS[out], resolution, n)
        assert self.b, "cfhd_amd_decode_batch_create -> NULL (%s)" % amd_last_error()
        w = ctypes.c_int(); h = ctypes.c_int(); rb = ctypes.c_int()
        assert self.L.cfhd_amd_decode_batch_geometry(self.b, ctypes.byref(w), ctypes.byref(h), ctypes.byref(rb)) == 0
        self.w, self.h, self.row_bytes = w.value, h.value, rb.value

    def submit(self, blob, offsets, sizes, pictures=None, stride=0, pitch=0):
        self.keep = (blob, pictures)
        return self.L.cfhd_amd_decode_batch_submit_host(self.b, blob.ctypes.data_as(V), _sizes(offsets), _sizes(sizes), len(offsets),
                                                        pictures.ctypes.data_as(V) if pictures is not None else None, stride, pitch)

    def wait(self, count):
        status = (ctypes.c_int * count)(*([77] * count))
        return self.L.cfhd_amd_decode_batch_wait(self.b, status), list(status)

    def decode(self, samples, sizes=None):
        """One synchronous pass from plain memory, the pictures left in HBM: (wait's value, statuses, pictures)."""
        blob, offsets, sizes = pack(samples, sizes)
        assert self.submit(blob, offsets, sizes) == 0, amd_last_error()
        ret, status = self.wait(len(samples))
        return ret, status, self.pictures(len(samples))

    def pictures(self, count):
        out = []
        for i in range(count):
            o = np.full(self.row_bytes * self.h, 7, np.uint8)
            assert self.L.cfhd_amd_decode_batch_download_output(self.b, i, o.ctypes.data_as(V), self.row_bytes) == 0, amd_last_error()
            out.append(o)
        return out

    def close(self):
        if self.b: self.L.cfhd_amd_decode_batch_destroy(self.b); self.b = None


def handle_pictures(samples, out, resolution, sizes=None, first=None):
    """The yardstick: [(return code, picture)] of CFHD_DecodeSample through one handle prepared on the whole first sample, and the picture's (w, h, row bytes)."""
    L = product()
    dec = V(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        first = first if first is not None else samples[0]
        aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
        fb = ctypes.create_string_buffer(first, len(first))
        rc = L.CFHD_PrepareToDecode(dec, 0, 0, FOURCCS[out], resolution, 0, fb, len(first), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af))
        assert rc == 0, "CFHD_PrepareToDecode -> %d" % rc
        p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
        # the row bytes of a packed picture (what the queue reports): CFHD_GetImagePitch rounds up to 16 bytes
        px = ctypes.c_uint32(); L.CFHD_GetPixelSize(af.value, ctypes.byref(px))
        row = p.value if out == "v210" else aw.value * px.value
        res = []
        for k, s in enumerate(samples):
            sb = ctypes.create_string_buffer(s, len(s)); pic = np.full(row * ah.value, 7, np.uint8)
            rc = L.CFHD_DecodeSample(dec, sb, sizes[k] if sizes is not None else len(s), pic.ctypes.data_as(V), row)
            res.append((rc, pic))
        return res, (aw.value, ah.value, row)
    finally:
        L.CFHD_CloseDecoder(dec)


_cache = {}


def _yuy2_frame(w, h, i, interlaced):
    if not interlaced: return synth_yuy2(w, h, 20 + i)[0]
    f = field_flicker_frame(w, h)[0].reshape(h, w * 2)
    return np.ascontiguousarray(np.roll(f, 4 * 5 * i, axis=1)).reshape(-1)      # (whole YUYV quads: the picture moves, the layout stays)


def samples_of(kind, w, h, source, quality=QUALITY_FILMSCAN1, n=8):
    """n samples of n distinct frames from the reference's encoder ("ref") or the product's ("amd"); encoded once, shared, read-only."""
    key = (kind, w, h, source, quality, n, bool(use_emulated()))
    if key not in _cache:
        import gop_input_frames
        if kind in ("422", "422i"): frames, pitch, pix, enc, flags = [_yuy2_frame(w, h, i, kind == "422i") for i in range(n)], w * 2, PIX_YUY2, ENCODED_YUV422, int(kind == "422i")
        elif kind == "444": (frames, pitch), pix, enc, flags = gop_input_frames.frames("RG48", w, h, n), PIX_RG48, ENCODED_RGB444, 0
        else: (frames, pitch), pix, enc, flags = gop_input_frames.frames("b64a", w, h, n), PIX_B64A, ENCODED_RGBA4444, 0
        encode = ref_encode_frames if source == "ref" else amd_encode_frames
        _cache[key] = encode([np.ascontiguousarray(f) for f in frames], pitch, w, h, pix, enc, quality, flags)
    return _cache[key]


def use_emulated():
    import cfhd_testlib
    return cfhd_testlib._use_emulated_product


def _same(a, b, what):
    assert np.array_equal(a, b), "%s: %d bytes differ from the handle's picture" % (what, int((a != b).sum()))


# ---- 1. foreign samples
def check_foreign_exact(kind, w, h, out, resolution, source):
    samples = samples_of(kind, w, h, source)
    assert len(set(samples)) == len(samples) == 8
    want, geometry = handle_pictures(samples, out, resolution)
    q = Queue(samples[0], out, resolution, 8)
    try:
        assert (q.w, q.h, q.row_bytes) == geometry
        ret, status, pictures = q.decode(samples)
        assert ret == 8 and status == [0] * 8, (ret, status, amd_last_error())
        for i in range(8):
            assert want[i][0] == 0
            _same(pictures[i], want[i][1], "%s -> %s sample %d" % (kind, out, i))
    finally:
        q.close()


def check_foreign_dithered(kind, w, h, out, exact_out, source):
    samples = samples_of(kind, w, h, source)
    want, geometry = handle_pictures(samples, out, FULL)
    q = Queue(samples[0], out, FULL, 8)
    try:
        assert (q.w, q.h, q.row_bytes) == geometry
        for step in range(2):                                    # (the seed follows the pass number: both passes stay inside the step)
            ret, status, pictures = q.decode(samples)
            assert ret == 8 and status == [0] * 8, (ret, status, amd_last_error())
            for i in range(8):
                d = np.abs(pictures[i].astype(np.int16) - want[i][1].astype(np.int16))
                assert d.max() <= 1, "%s -> %s pass %d sample %d: %d bytes further than one step from the handle's" % (kind, out, step, i, int((d > 1).sum()))
    finally:
        q.close()
    check_foreign_exact(kind, w, h, exact_out, FULL, source)


def check_mixed_qualities(source):
    """One pass of samples of two qualities, FILMSCAN1 and a rate-feedback quality (FILMSCAN2: the tables move from sample to sample): the quantizers come from each sample."""
    w, h = 192, 96
    a, b = samples_of("422", w, h, source), samples_of("422", w, h, source, quality=5)
    assert len(set(len(s) for s in b)) > 1
    samples = [x for pair in zip(a[:4], b[4:]) for x in pair]
    want, _ = handle_pictures(samples, "YU64", FULL)
    q = Queue(samples[0], "YU64", FULL, 8)
    try:
        ret, status, pictures = q.decode(samples)
        assert ret == 8 and status == [0] * 8
        for i in range(8): _same(pictures[i], want[i][1], "mixed qualities, sample %d" % i)
    finally:
        q.close()


# ---- 2. ingest
def scattered_blob(samples, seed=3):
    """The samples in one blob in shuffled order, junk between them, sample i at an offset that is i mod 16 modulo 16: (blob, offsets, sizes)."""
    rng = np.random.default_rng(seed)
    order = list(rng.permutation(len(samples)))
    offsets = [0] * len(samples); at = int(rng.integers(1, 64)); parts = []
    blob = bytearray()
    for i in order:
        at = len(blob) + int(rng.integers(1, 200))
        at += (i % 16 - at) % 16
        blob += bytes(rng.integers(0, 256, at - len(blob), dtype=np.uint8))
        offsets[i] = at
        blob += samples[i]
    blob += bytes(rng.integers(0, 256, 37, dtype=np.uint8))
    assert sorted(o % 16 for o in offsets) == sorted(i % 16 for i in range(len(samples)))
    return np.frombuffer(bytes(blob), np.uint8).copy(), offsets, [len(s) for s in samples]


def device_copy(blob):
    """(owner, device pointer) of the blob in HBM; under the emulator, whose "device" pointers are the kernels' own address space, the blob itself."""
    if use_emulated(): return blob, blob.ctypes.data
    return DeviceBlob(blob), None


class DeviceBlob:
    """A copy of a host array in HBM on the device the library's batches live on, through the HIP runtime the product library has already loaded (hipMalloc /
    hipMemcpy / hipFree by ctypes: nothing else in the process needs to know the GPU)."""
    def __init__(self, blob):
        lib()                                                # (the product library brings the runtime in)
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.hip = ctypes.CDLL(path)
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(V), ctypes.c_size_t]; self.hip.hipFree.argtypes = [V]
        self.hip.hipMemcpy.argtypes = [V, V, ctypes.c_size_t, ctypes.c_int]; self.hip.hipSetDevice.argtypes = [ctypes.c_int]
        count = ctypes.c_int(); assert self.hip.hipGetDeviceCount(ctypes.byref(count)) == 0 and count.value > 0
        pinned = os.environ.get("CFHD_AMD_DEVICE") or os.environ.get("LOCAL_RANK")      # (cfhd_device.hip device_init)
        self.device = int(pinned) % count.value if pinned else 0
        assert self.hip.hipSetDevice(self.device) == 0
        self.ptr = V()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), blob.nbytes) == 0
        assert self.hip.hipMemcpy(self.ptr, blob.ctypes.data_as(V), blob.nbytes, 1) == 0      # hipMemcpyHostToDevice (synchronous)

    def __del__(self):
        if getattr(self, "ptr", None): self.hip.hipSetDevice(self.device); self.hip.hipFree(self.ptr); self.ptr = None


def check_ingest(source="ref"):
    w, h, out = 192, 96, "YU64"
    eight = samples_of("422", w, h, source)
    samples = [eight[i % 8] for i in range(17)]
    want, _ = handle_pictures(samples, out, FULL)
    blob, offsets, sizes = scattered_blob(samples)
    L = lib()
    q = Queue(samples[0], out, FULL, 17)
    try:
        row, frame = q.row_bytes, q.row_bytes * q.h
        # plain memory, the pictures to plain memory
        pics = np.full(frame * 17, 9, np.uint8)
        assert q.submit(blob, offsets, sizes, pics, frame, row) == 0, amd_last_error()
        assert q.wait(17) == (17, [0] * 17)
        for i in range(17): _same(pics[i * frame: (i + 1) * frame], want[i][1], "plain memory, sample %d" % i)
        # a registered blob, the pictures to registered memory
        pics2 = np.full(frame * 17, 9, np.uint8)
        assert L.cfhd_amd_register_host_buffer(blob.ctypes.data_as(V), blob.nbytes) == 0 and L.cfhd_amd_register_host_buffer(pics2.ctypes.data_as(V), pics2.nbytes) == 0
        try:
            assert q.submit(blob, offsets, sizes, pics2, frame, row) == 0, amd_last_error()
            assert q.wait(17) == (17, [0] * 17)
        finally:
            L.cfhd_amd_unregister_host_buffer(blob.ctypes.data_as(V)); L.cfhd_amd_unregister_host_buffer(pics2.ctypes.data_as(V))
        for i in range(17): _same(pics2[i * frame: (i + 1) * frame], want[i][1], "registered memory, sample %d" % i)
        # the blob in HBM
        owner, dptr = device_copy(blob)
        if dptr is None: dptr = owner.ptr
        assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, _sizes(offsets), _sizes(sizes), 17) == 0, amd_last_error()
        assert q.wait(17) == (17, [0] * 17)
        for i, p in enumerate(q.pictures(17)): _same(p, want[i][1], "device memory, sample %d" % i)
        # a sample that leaves the span is refused, not read
        assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, offsets[0] + sizes[0] - 1, _sizes(offsets[:1]), _sizes(sizes[:1]), 1) == -1
        del owner
    finally:
        q.close()


def check_short_samples_after_long_ones(source="ref"):
    """The zeroed tail: a pass of short samples in slots that held long ones decodes as on a fresh batch."""
    w, h, out = 192, 96, "YU64"
    rng = np.random.default_rng(11)
    noisy = [rng.integers(0, 256, w * 2 * h, dtype=np.uint8) for _ in range(8)]
    flat = [np.full(w * 2 * h, 100 + 5 * i, np.uint8) for i in range(8)]
    encode = ref_encode_frames if source == "ref" else amd_encode_frames
    long_ones, short_ones = encode(noisy, w * 2, w, h), encode(flat, w * 2, w, h)
    assert min(len(s) for s in long_ones) > 4 * max(len(s) for s in short_ones)
    want_long, _ = handle_pictures(long_ones, out, FULL); want_short, _ = handle_pictures(short_ones, out, FULL, first=long_ones[0])
    q = Queue(long_ones[0], out, FULL, 8); fresh = Queue(long_ones[0], out, FULL, 8)
    try:
        ret, status, pictures = q.decode(long_ones)
        assert ret == 8 and status == [0] * 8
        for i in range(8): _same(pictures[i], want_long[i][1], "long sample %d" % i)
        ret, status, pictures = q.decode(short_ones)
        ret2, status2, pictures2 = fresh.decode(short_ones)
        assert ret == ret2 == 8 and status == status2 == [0] * 8
        for i in range(8):
            _same(pictures[i], want_short[i][1], "short sample %d behind a long one" % i)
            _same(pictures2[i], pictures[i], "short sample %d on a fresh batch" % i)
    finally:
        q.close(); fresh.close()


def check_short_pass_leaves_the_rest_alone(source="ref"):
    """count = 3 of nsamples = 8, a pitch wider than the rows: nothing behind a row's bytes, nothing for pictures 3 .. 7."""
    w, h, out = 192, 96, "YU64"
    samples = samples_of("422", w, h, source)
    want, _ = handle_pictures(samples[:3], out, FULL)
    q = Queue(samples[0], out, FULL, 8)
    try:
        pitch = q.row_bytes + 32; frame = pitch * q.h + 64
        for registered in (False, True):
            pics = np.full(frame * 8, 0x5a, np.uint8)
            if registered: assert q.L.cfhd_amd_register_host_buffer(pics.ctypes.data_as(V), pics.nbytes) == 0
            try:
                blob, offsets, sizes = pack(samples[:3])
                assert q.submit(blob, offsets, sizes, pics, frame, pitch) == 0, amd_last_error()
                assert q.wait(3) == (3, [0, 0, 0])
            finally:
                if registered: q.L.cfhd_amd_unregister_host_buffer(pics.ctypes.data_as(V))
            for i in range(3):
                img = pics[i * frame: i * frame + pitch * q.h].reshape(q.h, pitch)
                _same(img[:, : q.row_bytes].reshape(-1), want[i][1], "picture %d" % i)
                assert (img[:, q.row_bytes:] == 0x5a).all(), "picture %d: bytes behind the rows were written" % i
                assert (pics[i * frame + pitch * q.h: (i + 1) * frame] == 0x5a).all()
            assert (pics[3 * frame:] == 0x5a).all(), "pictures behind the count were written"
    finally:
        q.close()


# ---- 3. verdicts
def walk_bands(sample):
    """[(position of the size chunk, position behind the band header, end of the chunk)] of every coded band, by the tag walk of parse_sample."""
    d = sample; pos = 0; pending_at = pending = chunk_pos = 0; out = []
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
        elif tag == 4 and value == 0x0f0f: pos = pending_at + pending
        elif tag == 55: out.append((chunk_pos, pos, pending_at + pending)); pos = pending_at + pending
    return out


def damaged(kind, sample, other):
    """(bytes, size handed to the decoder) of sample 3 of the pass: the deterministic kinds of test_gpu_parity.test_decoder_survives_fuzzed_samples."""
    s = bytearray(sample)
    if kind == "cut in half": return bytes(s), (len(s) // 2) & ~3
    if kind == "frame width":
        at = next(p for p in range(0, 512, 4) if s[p: p + 2] == b"\x00\x14")      # TAG_FRAME_WIDTH
        v = int.from_bytes(s[at + 2: at + 4], "big") + 16; s[at + 2: at + 4] = v.to_bytes(2, "big")
        return bytes(s), len(s)
    bands = walk_bands(sample)
    assert len(bands) == 27
    if kind == "size chunk":
        at = bands[-1][0]; s[at: at + 4] = b"\x20\xff\xff\xff"
        return bytes(s), len(s)
    if kind == "payload pattern":
        _, lo, hi = max(bands, key=lambda b: b[2] - b[1])
        at = (lo + (hi - lo) // 2) & ~3; s[at: at + 64] = bytes((i * 37 + 11) & 0xff for i in range(64))
        return bytes(s), len(s)
    if kind == "other geometry": return other, len(other)
    if kind == "two bytes": return bytes(s[:2]), 2
    raise ValueError(kind)


def check_verdicts(kind, source="ref"):
    w, h, out = 192, 96, "YU64"
    samples = list(samples_of("422", w, h, source))
    other = samples_of("422", 208, 104, source, n=1)[0]
    intact = list(samples)
    samples[3], size3 = damaged(kind, samples[3], other)
    sizes = [len(s) for s in samples]; sizes[3] = size3
    want, _ = handle_pictures(samples, out, FULL, sizes=sizes)
    print("%s: the handle answers %d" % (kind, want[3][0]))
    assert [rc for i, (rc, _) in enumerate(want) if i != 3] == [0] * 7
    q = Queue(intact[0], out, FULL, 8)
    try:
        # the samples at their own lengths in the blob, sample 3 with the size the decoder is told
        blob, offsets, _ = pack(samples)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        ret, status = q.wait(8)
        pictures = q.pictures(8)
        assert status == [rc for rc, _ in want], (status, [rc for rc, _ in want])
        assert ret == status.count(0)
        for i in range(8):
            _same(pictures[i], want[i][1], "%s: sample %d" % (kind, i))
            if status[i]: assert not pictures[i].any(), "sample %d failed and its picture is not zero" % i
        # the same pass with its pictures to host memory: the host pictures and download_output both agree with the statuses
        frame = q.row_bytes * q.h; host = np.full(frame * 8, 9, np.uint8)
        assert q.submit(blob, offsets, sizes, host, frame, q.row_bytes) == 0, amd_last_error()
        ret2, status2 = q.wait(8)
        assert (ret2, status2) == (ret, status)
        for i, p in enumerate(q.pictures(8)):
            _same(host[i * frame: (i + 1) * frame], want[i][1], "%s: host picture %d" % (kind, i))
            _same(p, want[i][1], "%s: download_output(%d) behind a pass with host pictures" % (kind, i))
        # an intact pass on the same batch afterwards
        good, _ = handle_pictures(intact, out, FULL)
        ret, status, pictures = q.decode(intact)
        assert ret == 8 and status == [0] * 8
        for i in range(8): _same(pictures[i], good[i][1], "intact pass behind '%s': sample %d" % (kind, i))
    finally:
        q.close()
    return want[3][0]


# ---- 4. queue
def check_queue(source="ref"):
    w, h, out = 192, 96, "YU64"
    sets = [samples_of("422", w, h, source), samples_of("422i", w, h, source)]
    want = [handle_pictures(s, out if k == 0 else "RG48", FULL)[0] for k, s in enumerate(sets)]
    L = lib()
    qs = [Queue(sets[0][0], out, FULL, 8), Queue(sets[1][0], "RG48", FULL, 8)]
    try:
        packed = [pack(s) for s in sets]
        for step in range(2):
            for q, (blob, offsets, sizes) in zip(qs, packed): assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
            q = qs[0]; blob, offsets, sizes = packed[0]
            buf = np.zeros(q.row_bytes * q.h, np.uint8); x = ctypes.c_int()
            assert q.submit(blob, offsets, sizes) == -1
            assert L.cfhd_amd_decode_batch_submit_device(q.b, blob.ctypes.data_as(V), blob.nbytes, _sizes(offsets), _sizes(sizes), 8) == -1
            assert L.cfhd_amd_decode_batch_geometry(q.b, ctypes.byref(x), None, None) == -1
            assert L.cfhd_amd_decode_batch_download_output(q.b, 0, buf.ctypes.data_as(V), q.row_bytes) == -1
            assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 0) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 0) == b""
            for k, q in enumerate(qs):
                assert q.wait(8) == (8, [0] * 8)
                for i, p in enumerate(q.pictures(8)): _same(p, want[k][i][1], "batch %d step %d sample %d" % (k, step, i))
            assert L.cfhd_amd_decode_batch_wait(qs[0].b, None) == -1                  # nothing in flight
        names = [L.cfhd_amd_decode_batch_kernel_name(qs[0].b, k).decode() for k in range(8)]
        assert names[0] == "k_dec_ingest" and names[1] == "k_dec_parse" and names[7] == "k_dec_blank" and all(names), names
        # (every slot answers; a kernel that leaves after one load -- k_dec_blank over clean samples -- may last less than the event clock resolves, so the sum is held, not each)
        ms = [L.cfhd_amd_decode_batch_kernel_ms(qs[0].b, k) for k in range(8)]
        assert all(x >= 0 for x in ms) and sum(ms) > 0 and L.cfhd_amd_decode_batch_kernel_ms(qs[0].b, 8) == 0, ms
        # destroy on a batch in flight returns
        blob, offsets, sizes = packed[1]
        assert qs[1].submit(blob, offsets, sizes) == 0
        qs[1].close()
    finally:
        for q in qs: q.close()


# ---- 5. gates
def refused(sample, out, resolution, n):
    L = lib()
    fb = ctypes.create_string_buffer(sample, len(sample))
    b = L.cfhd_amd_decode_batch_create(fb, len(sample), FOURCCS[out], resolution, n)
    if b: L.cfhd_amd_decode_batch_destroy(b); return False
    text = amd_last_error()
    assert text, "refused without a text"
    return text


def check_gates():
    w, h = 192, 96
    progressive = samples_of("422", w, h, "amd", n=2)
    interlaced = samples_of("422i", w, h, "amd", n=2)
    frames = [synth_yuy2(w, h, 20 + i)[0] for i in range(2)]
    group_stream = amd_encode_frames(frames, w * 2, w, h, PIX_YUY2, flags=ENCODING_FLAGS_2FRAME_GOP)
    assert len(group_stream[0]) == 40
    assert "group" in refused(group_stream[0], "YUY2", FULL, 4), "a sequence header"
    assert "group" in refused(group_stream[1], "YUY2", FULL, 4), "a group sample"
    mosaic = synth_bayer(w, h, 7).reshape(-1).view(np.uint8).copy()
    bayer = amd_encode_frames([mosaic], w * 2, w, h, PIX_BYR4, ENCODED_BAYER)[0]
    assert "Bayer" in refused(bayer, "BYR4", FULL, 4)
    assert "CFHD_Error 11" in refused(progressive[0], "YUY2", QUARTER, 4), "quarter resolution"
    assert "CFHD_Error 3" in refused(progressive[0], "r210", FULL, 4), "r210 of a 4:2:2 sample"
    assert "CFHD_Error 3" in refused(interlaced[0], "RG24", FULL, 4), "RG24 of an interlaced sample"
    assert "nsamples" in refused(progressive[0], "YUY2", FULL, 0)
    # a sample of the uncompressed mode: the first band's size chunk made an UNCOMPRESS chunk (0x23xx); the handle's own text comes through
    raw = bytearray(progressive[0]); at = walk_bands(progressive[0])[0][0]; raw[at: at + 4] = b"\x23\x00\x00\x01"
    assert "uncompressed" in refused(bytes(raw), "YUY2", FULL, 4)
    q = Queue(progressive[0], "YUY2", FULL, 2); q.close()      # (and the same arguments with a count are served)


def gates_under_host_entropy():
    """Child process body (CFHD_AMD_ENTROPY=host is read when the library starts its first encoder): the queue refuses, the handle still decodes."""
    w, h = 192, 96
    sample = amd_encode_frames([synth_yuy2(w, h, 20)[0]], w * 2, w, h)[0]
    text = refused(sample, "YUY2", FULL, 4)
    assert text and "CFHD_AMD_ENTROPY" in text, text
    amd_decode_sample(sample)
    print("HOST ENTROPY REFUSED")
