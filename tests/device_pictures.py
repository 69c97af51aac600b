"""The device-memory side of the two queues: cfhd_amd_decode_batch_set_device_pictures (the pictures of a pass into device memory the caller owns, packed or as planar
R, G, B tensors of u16 / f16 / f32, written by k_dec_deliver) and cfhd_amd_batch_upload_device (frames that lie in HBM into the frame queue).  The helpers and test
bodies shared by tests/test_gpu_device_pictures.py (hardware) and tests/test_device_pictures_emulated.py (the same functions inside cfhd_testlib.emulated_product(),
where a device pointer is a host pointer).

Every comparison is exact.  The yardstick for picture contents is the decode queue suites': one CFHD_DecodeSample handle fed the same samples
(decode_queue.handle_pictures); for the outputs with a dither step, cfhd_amd_decode_batch_download_output of the same pass.  The planar tensors expected are numpy on the
handle's RG48 words w: u16 w, f32 w.astype(float32) * (float32(1) / float32(65535)), f16 that .astype(float16); the float layouts are compared as bit patterns.
A device buffer is checked whole: it is filled with a pattern, guard regions in front and behind, and after a pass it has to equal the pattern with exactly the row
bytes of the pictures replaced -- every byte of pitch padding, of the gaps between planes and pictures, of the pictures behind a short pass and of the guards included.
Test infrastructure only."""
import ctypes, os, subprocess
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import group_decode_queue as GQ
from decode_queue import samples_of, handle_pictures, scattered_blob, damaged, DeviceBlob, use_emulated, FULL, HALF, V, _sizes

PACKED, PLANAR_U16, PLANAR_F16, PLANAR_F32 = 0, 1, 2, 3
LAYOUT_NAMES = {PACKED: "packed", PLANAR_U16: "u16", PLANAR_F16: "f16", PLANAR_F32: "f32"}
ELEMENT = {PLANAR_U16: 2, PLANAR_F16: 2, PLANAR_F32: 4}
GUARD = 256

# 1. packed: (name, intra kind or "groups", w, h, output, resolution, exact).  One case per family of the last launch -- a 4:2:2 output with no conversion behind it,
# v210, a 16-bit RGB output of a 4:2:2 sample, a 10-bit RGB word output of a 4:4:4 sample, b64a of a 4:4:4:4 sample --, one at half resolution, one that dithers (its
# yardstick: download_output of the same pass), progressive groups to YU64, and rows that are no multiple of 16 bytes long (RG24 of a 4:4:4 sample 200 pixels wide:
# 600 bytes, the kernel's narrower tail; RG24 dithers)
PACKED_CASES = [("yu64", "422", 320, 240, "YU64", FULL, True), ("v210", "422", 192, 96, "v210", FULL, True), ("rg48-of-422", "422", 208, 104, "RG48", FULL, True),
                ("dpx0-of-444", "444", 208, 104, "DPX0", FULL, True), ("b64a-of-4444", "4444", 192, 96, "b64a", FULL, True), ("yuy2-half", "422", 320, 240, "YUY2", HALF, True),
                ("yuy2-dithered", "422", 320, 240, "YUY2", FULL, False), ("groups-yu64", "groups", 320, 240, "YU64", FULL, True), ("rg24-600-byte-rows", "444", 200, 64, "RG24", FULL, False)]
# 2. planar, all to RG48: (name, kind, w, h, resolution).  24 lanes a row (a partial wave), 12 lanes, 66 lanes (a row crosses a wave), an RGBA sample, interlaced groups,
# and the one family whose width is no multiple of 8: RGB 4:4:4 at half resolution, 100 pixels -- rows that start off 16-byte boundaries, four tail columns.
# That last case was added for the kernel's element-by-element path and is held to cfhd_amd_decode_batch_download_output of the same pass, not to the handle: on the
# hardware the batch decoder's own half-resolution RG48 pictures of a 4:4:4 sample 200 pixels wide differ from the handle's in a few hundred bytes a picture, with
# no device delivery set and on the code as it stood before this kernel existed (under the emulator the two agree, and the case is held to the handle there too).
# What k_dec_deliver has to show is that the caller's memory holds the pictures the pass decoded.
PLANAR_CASES = [("422-192x96", "422", 192, 96, FULL), ("422-half-96x48", "422", 192, 96, HALF), ("444-528x64", "444", 528, 64, FULL), ("4444-192x96", "4444", 192, 96, FULL),
                ("interlaced-groups-192x96", "groups-i", 192, 96, FULL), ("444-half-100x32", "444", 200, 64, HALF)]


def source():
    """The reference's samples where oracle/_ref is built, the product's otherwise."""
    return "ref" if have_ref() else "amd"


def lib():
    L = GQ.lib()
    if not getattr(L, "_device_pictures_declared", False):
        L.cfhd_amd_decode_batch_set_device_pictures.argtypes = [V, V, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
        L.cfhd_amd_batch_upload_device.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_batch_create_ex.restype = V
        L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32] + [ctypes.c_int] * 4
        L.cfhd_amd_batch_destroy.argtypes = [V]; L.cfhd_amd_batch_destroy.restype = None
        L.cfhd_amd_batch_upload.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_batch_roundtrip.restype = ctypes.c_longlong; L.cfhd_amd_batch_roundtrip.argtypes = [V]
        L.cfhd_amd_batch_get_sample.argtypes = [V, ctypes.c_int, ctypes.POINTER(V), ctypes.POINTER(ctypes.c_size_t)]
        L.cfhd_amd_set_clip_guid.argtypes = [ctypes.c_char_p]; L.cfhd_amd_set_clip_guid.restype = None
        L._device_pictures_declared = True
    return L


def pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.uint32) * 37 + 11) & 0xff).astype(np.uint8)


class DeviceArray:
    """`nbytes` of device memory on the library's device, 16-byte aligned, holding a copy of `host`: HBM through DeviceBlob on the hardware; under the emulator, whose
    device pointers are the kernels' own address space, an aligned numpy array."""
    def __init__(self, host):
        host = np.ascontiguousarray(host, np.uint8)
        self.nbytes = host.nbytes
        if use_emulated():
            raw = np.zeros(self.nbytes + 64, np.uint8)
            at = (-raw.ctypes.data) % 64
            self.array = raw[at: at + self.nbytes]; self.array[:] = host
            self.ptr = self.array.ctypes.data; self.blob = None
        else:
            self.blob = DeviceBlob(host)
            self.ptr = self.blob.ptr.value
        assert self.ptr % 16 == 0

    def read(self):
        if self.blob is None: return self.array.copy()
        out = np.empty(self.nbytes, np.uint8)
        assert self.blob.hip.hipSetDevice(self.blob.device) == 0
        assert self.blob.hip.hipMemcpy(out.ctypes.data_as(V), self.blob.ptr, self.nbytes, 2) == 0      # hipMemcpyDeviceToHost (synchronous)
        return out


# ---- the expected contents of a device buffer
def planar_bytes(picture, w, h, layout):
    """The three planes of an RG48 picture (h rows of 6 w bytes) in the element type of `layout`: uint8 [3, h, w * element size]."""
    words = picture.view(np.uint16).reshape(h, w, 3)
    planes = np.ascontiguousarray(words.transpose(2, 0, 1))
    if layout == PLANAR_U16: return planes.view(np.uint8).reshape(3, h, w * 2)
    f32 = planes.astype(np.float32) * (np.float32(1) / np.float32(65535))
    assert f32.dtype == np.float32
    if layout == PLANAR_F32: return np.ascontiguousarray(f32).view(np.uint8).reshape(3, h, w * 4)
    return np.ascontiguousarray(f32.astype(np.float16)).view(np.uint8).reshape(3, h, w * 2)


def geometry(q, layout, padded):
    """(row bytes of the layout, pitch, stride): the contiguous tensor geometry, or a pitch of row bytes (rounded up to 16) + 48 and a stride of picture + 4096."""
    row = q.row_bytes if layout == PACKED else q.w * ELEMENT[layout]
    planes = 1 if layout == PACKED else 3
    if not padded: pitch = (row + 15) & ~15; return row, pitch, planes * q.h * pitch
    pitch = ((row + 15) & ~15) + 48
    return row, pitch, planes * q.h * pitch + 4096


def put(expected, q, layout, pitch, stride, i, picture):
    """Picture i (the queue's packed bytes) where the layout puts it in a device buffer image that starts GUARD bytes in front of picture 0."""
    base = GUARD + i * stride
    if layout == PACKED:
        rows = picture.reshape(q.h, q.row_bytes)
        for r in range(q.h): expected[base + r * pitch: base + r * pitch + q.row_bytes] = rows[r]
        return
    planes = planar_bytes(picture, q.w, q.h, layout)
    row = planes.shape[2]
    for c in range(3):
        for r in range(q.h):
            at = base + (c * q.h + r) * pitch
            expected[at: at + row] = planes[c, r]


class Delivery:
    """A device buffer for `npictures` pictures of queue q in a layout and geometry, prefilled with the pattern, guards in front and behind."""
    def __init__(self, q, layout, padded, npictures):
        self.q, self.layout = q, layout
        self.row, self.pitch, self.stride = geometry(q, layout, padded)
        self.image = pattern(GUARD + npictures * self.stride + GUARD)
        self.mem = DeviceArray(self.image)

    def set(self):
        rc = lib().cfhd_amd_decode_batch_set_device_pictures(self.q.b, self.mem.ptr + GUARD, self.stride, self.pitch, self.layout)
        assert rc == 0, amd_last_error()

    def expect(self, pictures):
        """The buffer as it has to be once pictures[i] (None: untouched) were delivered on top of what it held."""
        for i, p in enumerate(pictures):
            if p is not None: put(self.image, self.q, self.layout, self.pitch, self.stride, i, p)
        return self.image

    def check(self, pictures, what):
        want, got = self.expect(pictures), self.mem.read()
        if np.array_equal(got, want): return
        bad = np.flatnonzero(got != want)
        rel = bad - GUARD
        inside = 0
        for i, p in enumerate(pictures):
            if p is None: continue
            mine = rel[(rel >= i * self.stride) & (rel < (i + 1) * self.stride)] - i * self.stride
            inside += int(((mine % self.pitch) < self.row).sum())
        raise AssertionError("%s: %d bytes of the device buffer differ (first at %d of %d); about %d of them in picture rows, the rest in padding, gaps or guards"
                             % (what, bad.size, int(bad[0]), got.size, inside))


# ---- the samples and the handle's pictures of a case: computed once, shared, read-only
_want = {}


_interlaced = {}


def interlaced_group_stream(w, h):
    """Four interlaced groups of textured frames (the field-flicker frames of group_decode_queue.group_stream decode to two distinct RG48 words, too few to tell the
    components of a plane apart), as group_stream hands them out: group, P-frame sample, group, ...; the sequence header dropped."""
    key = (w, h, source(), bool(use_emulated()))
    if key not in _interlaced:
        frames = [np.ascontiguousarray(synth_yuy2(w, h, 20 + i)[0]) for i in range(8)]
        encode = ref_encode_frames if source() == "ref" else amd_encode_frames
        stream = encode(frames + [frames[0]], w * 2, w, h, PIX_YUY2, ENCODED_YUV422, QUALITY_FILMSCAN1, GQ.GOP | 1)
        assert len(stream) == 9 and len(stream[0]) == 40 and all(len(s) == 24 for s in stream[2::2]), [len(s) for s in stream]
        _interlaced[key] = stream[1:]
    return _interlaced[key]


def case_samples(kind, w, h):
    if kind == "groups": return GQ.group_stream(source(), w, h, 0)
    if kind == "groups-i": return interlaced_group_stream(w, h)
    return samples_of(kind, w, h, source())


def case_queue(kind, samples, out, resolution):
    return GQ.GroupQueue(samples[0], out, resolution, 4) if kind.startswith("groups") else DQ.Queue(samples[0], out, resolution, 8)


def case_want(kind, w, h, out, resolution):
    key = (kind, w, h, out, resolution, source(), bool(use_emulated()))
    if key not in _want:
        res, geo = handle_pictures(case_samples(kind, w, h), out, resolution)
        assert [rc for rc, _ in res] == [0] * 8
        for _, p in res: p.setflags(write=False)
        _want[key] = ([p for _, p in res], geo)
    return _want[key]


def run_pass(q, samples, sizes=None, count=None):
    count = len(samples) if count is None else count
    blob, offsets, sz = DQ.pack(samples[:count], sizes[:count] if sizes is not None else None)
    assert q.submit(blob, offsets, sz) == 0, amd_last_error()
    return q.wait(count)


# ---- 1. packed
def check_packed(name, kind, w, h, out, resolution, exact):
    samples = case_samples(kind, w, h)
    q = case_queue(kind, samples, out, resolution)
    try:
        d = Delivery(q, PACKED, True, 8)
        assert d.pitch == ((q.row_bytes + 15) & ~15) + 48 and d.stride == q.h * d.pitch + 4096
        d.set()
        ret, status = run_pass(q, samples)
        assert ret == 8 and status == [0] * 8, (ret, status, amd_last_error())
        if exact:
            want, geo = case_want(kind, w, h, out, resolution)
            assert geo == (q.w, q.h, q.row_bytes)
        else: want = q.pictures(8)                              # (a dither step: the seed follows the pass, download_output of the same pass is the yardstick)
        assert len(set(p.tobytes() for p in want)) == 8
        d.check(want, "%s, packed" % name)
        # download_output beside device delivery: unchanged
        for i, p in enumerate(q.pictures(8)): assert np.array_equal(p, want[i]), "download_output(%d) beside device delivery" % i
    finally:
        q.close()


# ---- 2. planar
PASS_YARDSTICK = ("444-half-100x32",)


def check_planar(name, kind, w, h, resolution, layout):
    samples = case_samples(kind, w, h)
    want, geo = case_want(kind, w, h, "RG48", resolution)
    of_the_pass = name in PASS_YARDSTICK and not use_emulated()
    words = np.unique(np.concatenate([p.view(np.uint16) for p in want]))
    print("%s: %d distinct RG48 words in the 8 pictures" % (name, words.size))
    assert words.size >= 1000, "%s: only %d distinct words: pick other frames" % (name, words.size)
    q = case_queue(kind, samples, "RG48", resolution)
    try:
        assert geo == (q.w, q.h, q.row_bytes) and q.row_bytes == 6 * q.w
        for padded in (False, True):
            d = Delivery(q, layout, padded, 8)
            if not padded and q.w * ELEMENT[layout] % 16 == 0: assert d.pitch == q.w * ELEMENT[layout] and d.stride == 3 * q.h * q.w * ELEMENT[layout]      # a contiguous (8, 3, H, W) tensor
            d.set()
            ret, status = run_pass(q, samples)
            assert ret == 8 and status == [0] * 8, (ret, status, amd_last_error())
            if of_the_pass:
                want = q.pictures(8)
                assert np.unique(np.concatenate([p.view(np.uint16) for p in want])).size >= 1000
            d.check(want, "%s, %s, %s" % (name, LAYOUT_NAMES[layout], "pitch with padding" if padded else "contiguous tensor"))
    finally:
        q.close()


# ---- 3. the binary16 statement of the host-compiled build
F16_PROGRAM = r"""
// every RG48 word through the element rules of cfhd_deliver_kernels.h as a host compiler builds them: "word f32-bits f16-bits" per line
#include "hip_emu.h"
dim3 threadIdx, blockIdx, blockDim, gridDim;
#include "cfhd_deliver_kernels.h"
#include <stdio.h>
int main()
{
	for (unsigned w = 0; w < 65536u; w++) {
		const float f = cfhd::dev::deliver_unit_f32(w);
		unsigned bits; memcpy(&bits, &f, 4);
		printf("%u %u %u\n", w, bits, cfhd::dev::deliver_f16_bits(f));
	}
	// beyond the unit interval: the rule is stated for every single, so the carries and the ends are checked too
	const unsigned more[] = { 0x3f800000u, 0x3f801000u, 0x3f803000u, 0x477fe000u, 0x477ff000u, 0x47800000u, 0x7f800000u, 0x33000000u, 0x33000001u, 0x33800000u, 0x387fc000u, 0x387fe000u, 0x387ff000u, 0xb8000000u, 0x80000000u, 0x00000001u, 0x007fffffu };
	for (unsigned bits : more) { float f; memcpy(&f, &bits, 4); printf("x %u %u\n", bits, cfhd::dev::deliver_f16_bits(f)); }
	return 0;
}
"""


def check_binary16_statement():
    """All 65 536 words through the host-compiled conversion, against numpy's float32 -> float16 (round to nearest even, subnormals kept)."""
    build = os.path.join(ROOT, "tests", "_build"); os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(build, "deliver_f16_words.cpp"), os.path.join(build, "deliver_f16_words")
    header = os.path.join(PRODUCT_DIR, "csrc", "cfhd_deliver_kernels.h")
    if not os.path.exists(src) or open(src).read() != F16_PROGRAM: open(src, "w").write(F16_PROGRAM)
    cfhd_testlib_build_once(exe, ["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tests", "hipemu"), "-I" + os.path.join(PRODUCT_DIR, "csrc"), src], [src, header])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    table = np.array([[int(x) for x in line.split()] for line in lines[:65536]], dtype=np.uint32)
    assert table.shape == (65536, 3) and np.array_equal(table[:, 0], np.arange(65536))
    f32 = np.arange(65536, dtype=np.uint16).astype(np.float32) * (np.float32(1) / np.float32(65535))
    assert np.array_equal(table[:, 1], f32.view(np.uint32)), "the f32 rule"
    f16 = f32.astype(np.float16).view(np.uint16)
    bad = np.flatnonzero(table[:, 2] != f16)
    assert bad.size == 0, "binary16 of %d words differs from numpy's, first word %d: %#x, numpy %#x" % (bad.size, int(bad[0]), int(table[bad[0], 2]), int(f16[bad[0]]))
    assert (f16[1:4] < 0x0400).all() and f16[1] > 0, "words 1 .. 3 are binary16 subnormals"
    extra = [line.split() for line in lines[65536:] if line.startswith("x ")]
    assert len(extra) == 17
    with np.errstate(over="ignore"):
        for _, bits, got in extra:
            want = int(np.array([int(bits)], np.uint32).view(np.float32).astype(np.float16).view(np.uint16)[0])
            assert int(got) == want, "single %#x: %#x, numpy %#x" % (int(bits), int(got), want)


def cfhd_testlib_build_once(target, cmd, deps):
    import cfhd_testlib
    cfhd_testlib._build_once(target, cmd, deps)


# ---- 4. verdicts and the slow path
def check_verdicts(layout):
    """A damaged code stream (the band decoders' error word sends every sample the parser passed through the handle), a size that is no multiple of 4 (the slow path's by
    k_dec_ingest's mark) and a sample the device parser refuses for good: the device memory agrees with status[i] -- zeros where a sample failed, the handle's picture
    in the asked layout everywhere else."""
    w, h = 192, 96
    out = "YU64" if layout == PACKED else "RG48"
    intact = samples_of("422", w, h, source())
    samples = list(intact)
    samples[2], size2 = damaged("payload pattern", samples[2], None)
    samples[6], size6 = damaged("frame width", samples[6], None)
    sizes = [len(s) for s in samples]; sizes[2] = size2; sizes[6] = size6
    sizes[4] -= 2
    assert sizes[4] % 4 == 2
    res, geo = handle_pictures(samples, out, FULL, sizes=sizes, first=intact[0])
    codes = [rc for rc, _ in res]
    print("the handle answers", codes)
    assert codes[6] != 0 and codes.count(0) >= 5
    q = DQ.Queue(intact[0], out, FULL, 8)
    try:
        d = Delivery(q, layout, True, 8); d.set()
        ret, status = run_pass(q, samples, sizes)
        assert status == codes, (status, codes)
        assert ret == codes.count(0)
        want = [p if rc == 0 else np.zeros_like(p) for rc, p in res]
        for (rc, p) in res:
            if rc: assert not p.any()                          # (the handle zero-fills what it refuses)
        d.check(want, "verdicts, %s" % LAYOUT_NAMES[layout])
        # an intact pass on the same batch and buffer afterwards
        good, _ = case_want("422", w, h, out, FULL)
        ret, status = run_pass(q, intact)
        assert ret == 8 and status == [0] * 8
        d.check(good, "an intact pass behind the damaged one, %s" % LAYOUT_NAMES[layout])
    finally:
        q.close()


# ---- 5. a short pass, switching off
def check_short_pass_and_off():
    w, h, out = 192, 96, "YU64"
    samples = samples_of("422", w, h, source())
    want, _ = case_want("422", w, h, out, FULL)
    q = DQ.Queue(samples[0], out, FULL, 8)
    try:
        d = Delivery(q, PACKED, True, 8); d.set()
        ret, status = run_pass(q, samples, count=3)
        assert (ret, status) == (3, [0] * 3)
        d.check(want[:3] + [None] * 5, "count = 3 of 8")
        # submit_device delivers too
        blob, offsets, sizes = scattered_blob(samples[5:8] + samples[:2])
        mem = DeviceArray(blob)
        assert q.L.cfhd_amd_decode_batch_submit_device(q.b, mem.ptr, blob.nbytes, _sizes(offsets), _sizes(sizes), 5) == 0, amd_last_error()
        assert q.wait(5) == (5, [0] * 5)
        d.check(want[5:8] + want[:2] + [None] * 3, "submit_device, count = 5 of 8")
        # switched off: a further pass leaves the whole buffer alone, and its pictures are where they were before the feature
        assert lib().cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        ret, status = run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check([None] * 8, "after set_device_pictures(NULL)")
        for i, p in enumerate(q.pictures(8)): assert np.array_equal(p, want[i])
        assert q.L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0
    finally:
        q.close()


# ---- 6. gates
def check_gates():
    w, h = 192, 96
    samples = samples_of("422", w, h, source())
    L = lib()
    q = DQ.Queue(samples[0], "YU64", FULL, 8); q48 = DQ.Queue(samples[0], "RG48", FULL, 8)
    try:
        d = Delivery(q, PACKED, True, 8); d48 = Delivery(q48, PLANAR_F32, True, 8)
        p, p48 = d.mem.ptr + GUARD, d48.mem.ptr + GUARD
        def refused(queue, ptr, stride, pitch, layout, what):
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, ptr, stride, pitch, layout) == -1, what
            text = amd_last_error()
            assert text and "decode queue" in text, "%s: refused without a text" % what
            return text
        texts = [refused(q, p, d.stride, d.pitch, 4, "an unknown layout"), refused(q, p, d.stride, d.pitch, -1, "a negative layout"),
                 refused(q, p, d.stride, d.pitch, PLANAR_U16, "a planar layout on a YU64 batch"),
                 refused(q, p + 8, d.stride, d.pitch, PACKED, "a pointer off 16"), refused(q, p, d.stride + 8, d.pitch, PACKED, "a stride off 16"),
                 refused(q, p, d.stride, d.pitch + 8, PACKED, "a pitch off 16"),
                 refused(q, p, d.stride, q.row_bytes - 16, PACKED, "a pitch below the row bytes"), refused(q, p, d.stride, -d.pitch, PACKED, "a negative pitch"),
                 refused(q, p, d.pitch * (q.h - 1) + q.row_bytes - 16, d.pitch, PACKED, "a stride below one picture"),
                 refused(q48, p48, d48.stride, q48.w * 4 - 16, PLANAR_F32, "a pitch below the f32 row bytes"),
                 refused(q48, p48, d48.pitch * (3 * q48.h - 1) + q48.w * 4 - 16, d48.pitch, PLANAR_F32, "a stride below three planes")]
        assert len(set(texts)) == 5, texts
        # the smallest stride and pitch are served; a pass in flight refuses
        assert L.cfhd_amd_decode_batch_set_device_pictures(q48.b, p48, d48.pitch * (3 * q48.h - 1) + q48.w * 4, d48.pitch, PLANAR_F32) == 0, amd_last_error()
        d.set()
        blob, offsets, sizes = DQ.pack(samples)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        refused(q, p, d.stride, d.pitch, PACKED, "a pass in flight")
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == -1 and amd_last_error()
        assert q.wait(8) == (8, [0] * 8)
        want, _ = case_want("422", w, h, "YU64", FULL)
        d.check(want, "the pass the refused calls were made in")
        ms, name = L.cfhd_amd_decode_batch_kernel_ms(q.b, 9), L.cfhd_amd_decode_batch_kernel_name(q.b, 9)
        print("k_dec_deliver: %.4f ms" % ms)
        assert ms > 0 and name == b"k_dec_deliver", (ms, name)
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 7) == b"k_dec_blank" and L.cfhd_amd_decode_batch_kernel_ms(q.b, 8) == 0
    finally:
        q.close(); q48.close()


# ---- 7. the frame queue fed from device memory
GUID = b"device-pictures!"


def mask_clock(sample):
    """cfhd_testlib.mask_volatile_metadata without the GUID: the payloads of the DATE / TIME / TIMC tuples of the sample's metadata chunks zeroed, nothing else."""
    import cfhd_testlib
    b = bytearray(sample)
    for lo, size in cfhd_testlib._metadata_chunks(bytes(sample)):      # (none in the 24-byte P-frame sample of a group: compared as it is)
        chunk = bytes(b[lo: lo + size]); at = 0
        while at + 8 <= len(chunk):                              # tuples: FourCC, 24-bit little-endian size + type byte, payload padded to a longword
            tag = chunk[at: at + 4]; tsize = chunk[at + 4] | (chunk[at + 5] << 8) | (chunk[at + 6] << 16)
            if tag in (b"DATE", b"TIME", b"TIMC"):
                for k in range(min(tsize, len(chunk) - at - 8)): b[lo + at + 8 + k] = 0
            at += 8 + (tsize + 3) // 4 * 4
    return bytes(b)


def batch_samples(L, b, n):
    """The samples of the last pass, byte for byte but for the wall-clock tuples of their metadata (two batches that run on either side of a full second write different
    TIME strings: mask_clock; the clip GUID is fixed by encode_batch and is compared)."""
    out = []
    for i in range(n):
        p = V(); size = ctypes.c_size_t()
        assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(size)) == 0
        out.append(mask_clock(ctypes.string_at(p, size.value)))
    return out


def encode_batch(pix, encoded, flags, w, h, n, feed):
    """The samples of one pass of a mode-1 batch whose frames `feed(L, batch)` puts in place."""
    L = lib()
    L.cfhd_amd_set_clip_guid(GUID)
    b = L.cfhd_amd_batch_create_ex(w, h, pix, encoded, flags, QUALITY_FILMSCAN1, n, 1, 1)
    assert b, "cfhd_amd_batch_create_ex -> NULL (%s)" % amd_last_error()
    try:
        feed(L, b)
        total = L.cfhd_amd_batch_roundtrip(b)
        assert total > 0, (total, amd_last_error())
        samples = batch_samples(L, b, n)
        return samples
    finally:
        L.cfhd_amd_batch_destroy(b)


def check_upload_device(name, negative_pitch):
    import gop_input_frames
    w, h = 192, 96
    if name == "RG48": (frames, row), pix, encoded, flags, n = gop_input_frames.frames("RG48", w, h, 4), PIX_RG48, ENCODED_RGB444, 0, 4
    else: frames, row, pix, encoded, flags, n = [DQ._yuy2_frame(w, h, i, False) for i in range(4)], w * 2, PIX_YUY2, ENCODED_YUV422, (GQ.GOP if name == "YUY2 groups" else 0), 4
    frames = [np.ascontiguousarray(f).view(np.uint8).reshape(h, row) for f in frames]
    def host_feed(L, b):
        for i, f in enumerate(frames): assert L.cfhd_amd_batch_upload(b, i, f.ctypes.data_as(V), row) == 0
    first = encode_batch(pix, encoded, flags, w, h, n, host_feed)
    assert len(set(first)) == n
    # the same frames in device memory at a pitch wider than the rows, guards around them
    pitch = row + 64; stride = h * pitch + 512
    image = pattern(GUARD + n * stride + GUARD)
    for i, f in enumerate(frames):
        for r in range(h): image[GUARD + i * stride + r * pitch: GUARD + i * stride + r * pitch + row] = f[r]
    mem = DeviceArray(image)
    def device_feed(L, b):
        assert L.cfhd_amd_batch_upload_device(b, n, mem.ptr, pitch) == -1 and L.cfhd_amd_batch_upload_device(b, -1, mem.ptr, pitch) == -1, "a frame outside the batch"
        assert L.cfhd_amd_batch_upload_device(b, 0, None, pitch) == -1, "no pointer"
        assert L.cfhd_amd_batch_upload_device(b, 0, mem.ptr, row - 16) == -1, "a pitch below the row bytes"
        for i in range(n):
            at = mem.ptr + GUARD + i * stride
            # (a negative pitch: the pointer names the last row in memory, the rows are read in memory order -- Codec/encoder.c:1957)
            rc = L.cfhd_amd_batch_upload_device(b, i, at + (h - 1) * pitch, -pitch) if negative_pitch else L.cfhd_amd_batch_upload_device(b, i, at, pitch)
            assert rc == 0, amd_last_error()
    second = encode_batch(pix, encoded, flags, w, h, n, device_feed)
    for i in range(n): assert second[i] == first[i], "%s: sample %d of the batch fed from device memory differs (%d / %d bytes)" % (name, i, len(second[i]), len(first[i]))
    assert np.array_equal(mem.read(), image), "the source was written to"


# ---- 8. the chain, all in HBM: decode queue -> device pictures -> frame queue
def check_chain():
    w, h = 192, 96
    samples = samples_of("422", w, h, source())
    want, _ = case_want("422", w, h, "YU64", FULL)
    q = DQ.Queue(samples[0], "YU64", FULL, 8)
    try:
        d = Delivery(q, PACKED, True, 8); d.set()
        ret, status = run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        def device_feed(L, b):
            for i in range(8): assert L.cfhd_amd_batch_upload_device(b, i, d.mem.ptr + GUARD + i * d.stride, d.pitch) == 0, amd_last_error()
        chained = encode_batch(PIX_YU64, ENCODED_YUV422, 0, w, h, 8, device_feed)
    finally:
        q.close()
    def host_feed(L, b):
        for i in range(8): assert L.cfhd_amd_batch_upload(b, i, want[i].ctypes.data_as(V), q.row_bytes) == 0
    direct = encode_batch(PIX_YU64, ENCODED_YUV422, 0, w, h, 8, host_feed)
    assert len(set(direct)) == 8
    for i in range(8): assert chained[i] == direct[i], "sample %d of the chain differs from the sample of the handle's picture" % i
