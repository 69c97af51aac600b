"""RGB 4:4:4 and RGBA 4:4:4:4 samples delivered as the YU64 picture the reference decodes them to: cfhd_amd_decode_batch_set_device_pictures with
CFHD_AMD_PICTURES_RGB_AS_YU64 (the packed picture, the words Y0 Cr Y1 Cb) and _RGB_AS_YUV422_U16 / _F16 / _F32 (the same words as Y, Cb, Cr planes in the geometry of
the YUV422 layouts), written by k_dec_deliver_rgb_as_yuv out of the RG48 pictures of a pass.  The helpers and test bodies shared by tests/test_gpu_rgb_as_yuv.py
(hardware) and tests/test_rgb_as_yuv_emulated.py (the same functions inside cfhd_testlib.emulated_product(), where a device pointer is a host pointer).

Every comparison is exact; the float layouts are compared as bit patterns.  The witnesses are independent of the kernel:
  * a delivered picture is held to tests/rgb_as_yuv_model.py (numpy float32) on cfhd_amd_decode_batch_download_output of the same pass, with the matrix of the
    sample's own colour-space tag;
  * where oracle/_ref is built, the U16 and packed layouts are held to the reference decoder's YU64 picture of each sample as well (a decoder handle per sample,
    in a child process);
  * the mixed pass is held to a YU64 picture of the reference stored under tests/golden/ (make_golden below wrote it and its sample).
Device buffers are checked whole: filled with a pattern, guards in front and behind, and afterwards equal to the pattern with exactly the row bytes of the rows or
planes replaced.
Test infrastructure only."""
import ctypes, os, subprocess, sys, tempfile
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
import group_decode_queue as GQ
import device_pictures as DP
import gop_input_frames
import rgb_as_yuv_model as M
from device_pictures import DeviceArray, pattern, GUARD
from decode_queue import use_emulated, V, FULL, HALF, _sizes

PACKED = 0
RGB_AS_YU64, RGB_AS_YUV422_U16, RGB_AS_YUV422_F16, RGB_AS_YUV422_F32 = 15, 16, 17, 18
LAYOUTS = (RGB_AS_YU64, RGB_AS_YUV422_U16, RGB_AS_YUV422_F16, RGB_AS_YUV422_F32)
LAYOUT_NAMES = {RGB_AS_YU64: "yu64", RGB_AS_YUV422_U16: "u16", RGB_AS_YUV422_F16: "f16", RGB_AS_YUV422_F32: "f32"}
ELEMENT = {RGB_AS_YUV422_U16: 2, RGB_AS_YUV422_F16: 2, RGB_AS_YUV422_F32: 4}
DELIVER = b"k_dec_deliver_rgb_as_yuv"
SHAPE = (192, 96)
ZERO = "zero"                                                   # in a list of expected pictures: the picture of a sample that failed
FLAG_VIDEO_SYSTEMS = 1 << 8                                      # CFHD_ENCODING_FLAGS bit 8: the reference's encoder then tags the sample (tag 91) with bit 2 set
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_SAMPLE, GOLDEN_YU64 = os.path.join(GOLDEN, "rgb444_192x96_video_systems.cfhd"), os.path.join(GOLDEN, "rgb444_192x96_video_systems_yu64.npy")
# the texts of the library as it was before these layouts existed
PARENT_UNKNOWN = "decode queue: unknown layout of the device pictures"
PARENT_PLANAR = "decode queue: the planar layouts serve batches whose output is RG48"
PARENT_YUV422 = "decode queue: the 4:2:2 plane layouts serve batches whose output is YUY2, 2vuy or YU64"
PARENT_OFF_16 = "decode queue: the device pictures' pointer, stride and pitch are multiples of 16"
PARENT_LOW_PITCH = "decode queue: the device pictures' pitch is below the row bytes of the layout"
PARENT_LOW_STRIDE = "decode queue: the device pictures' stride is below what one picture occupies"
PARENT_U8_ON_YU64 = "decode queue: YUV422_U8 serves the 8-bit outputs YUY2 and 2vuy; a YU64 batch delivers YUV422_U16"


def lib(): return DP.lib()


# ---- frames and samples
PATCH_HI, PATCH_LO = 64900, 400
PATCHES = tuple(tuple(PATCH_HI if c else PATCH_LO for c in p) for p in ((1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)))


def _soften(plane):
    """A 7 x 7 box filter, the border replicated."""
    out = plane.astype(np.float64)
    for axis in (0, 1):
        padded = np.concatenate([np.repeat(np.take(out, [0], axis), 3, axis), out, np.repeat(np.take(out, [-1], axis), 3, axis)], axis)
        out = sum(np.take(padded, range(k, k + out.shape[axis]), axis) for k in range(7)) / 7.0
    return out


def patched_frames(fmt, w, h, n, seed=5):
    """n textured frames (gop_input_frames) of RG48 or b64a with a band of eight patches across the top quarter -- white, black, the primaries, yellow, cyan, magenta --
    that moves by a patch from frame to frame: under the video-systems matrix Y saturates at 65535 on white and Cb, Cr reach 0 on yellow and cyan (0.511 x (400 - 64900) +
    32768 < 0).  The patches stand at 64900 and 400 of 65535 and every edge is a ramp seven pixels long, the whole colour picture softened and kept inside those two
    levels: where a decoded component overshoots 16 bits beside a hard saturated edge, the reference decoder's own pictures are not a function of the sample (see
    REF_ATTEMPTS below) more often than anywhere else, and a test that holds anything to them keeps clear of that."""
    frames, pitch = gop_input_frames.frames(fmt, w, h, n, seed)
    words = 3 if fmt == "RG48" else 4
    out = []
    for i, f in enumerate(frames):
        px = np.array(f).view(np.uint16).reshape(h, w, words)
        for k in range(8):
            x0, x1 = (k * w) // 8, ((k + 1) * w) // 8
            px[: max(h // 4, 10), x0: x1, words - 3:] = PATCHES[(k + i) % 8]
        for c in range(words - 3, words): px[:, :, c] = np.clip(np.rint(_soften(px[:, :, c])), PATCH_LO, PATCH_HI).astype(np.uint16)
        out.append(np.ascontiguousarray(px).view(np.uint8).reshape(-1))
    return out, pitch


_samples = {}


def source(): return "ref" if have_ref() else "amd"


def samples_of(kind, w, h, n=8, flags=0, src=None, seed=5):
    """n samples of patched frames: kind "444" (RG48 -> RGB 4:4:4) or "4444" (b64a -> RGBA 4:4:4:4); encoded once, shared, read-only."""
    src = src or source()
    key = (kind, w, h, n, flags, src, seed, bool(use_emulated()))
    if key not in _samples:
        fmt, pix, enc = ("RG48", PIX_RG48, ENCODED_RGB444) if kind == "444" else ("b64a", PIX_B64A, ENCODED_RGBA4444)
        frames, pitch = patched_frames(fmt, w, h, n, seed)
        encode = ref_encode_frames if src == "ref" else amd_encode_frames
        _samples[key] = encode(frames, pitch, w, h, pix, enc, QUALITY_FILMSCAN1, flags)
    return _samples[key]


def tag_of(sample):
    t = M.color_space_tag(sample)
    return 0 if t is None else t


# ---- the reference's pictures.  Its threaded decoder is no function of the sample on every call: now and then a picture comes back with damaged stretches, a whole
# colour component at 0, or the green words beside a saturated edge wrapped (seen here on 8 cores for RGB 4:4:4 and RGBA 4:4:4:4 samples alike, in fresh processes
# more often than in a warm one; tests/test_oracle_vs_ref.py gives it six attempts against a deterministic picture for the same reason).  So the reference is asked in
# a child process of its own, a decoder handle per decode, and gets REF_ATTEMPTS decodes per picture to show the one that satisfies the exact statement it is held
# to; a damaged picture cannot satisfy it by accident, and when no attempt does, the caller fails with the counts.
REF_ATTEMPTS = 8


def _ref_decode(sample, w, h, pix):
    p, pitch = ref_decode_sample(sample, w, h, pix)
    return np.ascontiguousarray(p.reshape(h, pitch)[:, : w * (6 if pix == PIX_RG48 else 4)])


def _differ(a, b): return int((np.ascontiguousarray(a).view(np.uint16) != np.ascontiguousarray(b).view(np.uint16)).sum())


def _ref_child(src, dst):
    data = np.load(src, allow_pickle=False)
    w, h, n = int(data["w"]), int(data["h"]), int(data["n"])
    out = {}
    for i in range(n):
        s, tag = data["s%d" % i].tobytes(), int(data["tags"][i])
        if "want%d" % i in data.files:                           # the YU64 picture that equals a given one
            counts = []
            for k in range(REF_ATTEMPTS):
                yu = _ref_decode(s, w, h, PIX_YU64)
                counts.append(_differ(yu, data["want%d" % i]))
                if not counts[-1]: break
            out["yu64_%d" % i] = yu; out["counts%d" % i] = np.array(counts)
            continue
        rgs, yus, counts, found = [], [], [], None               # an RG48 and a YU64 picture of which the second is the model of the first
        for k in range(REF_ATTEMPTS):
            rgs.append(_ref_decode(s, w, h, PIX_RG48)); yus.append(_ref_decode(s, w, h, PIX_YU64))
            models = [M.yu64_of_rg48(rg, w, h, tag) for rg in rgs]
            pairs = [(_differ(m, yu), a, b) for a, m in enumerate(models) for b, yu in enumerate(yus) if a == k or b == k]
            counts.append(min(pairs)[0])
            if not counts[-1]: found = min(pairs); break
        _, a, b = found if found else (0, -1, -1)
        out["rg48_%d" % i] = rgs[a]; out["yu64_%d" % i] = yus[b]; out["counts%d" % i] = np.array(counts)
    np.savez(dst, **out)
    print("DECODED")


def _run_ref_child(samples, w, h, tags, want=None):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.npz"), os.path.join(d, "out.npz")
        arrays = {"s%d" % i: np.frombuffer(s, np.uint8) for i, s in enumerate(samples)}
        if want is not None: arrays.update({"want%d" % i: np.ascontiguousarray(p) for i, p in enumerate(want)})
        np.savez(src, w=w, h=h, n=len(samples), tags=np.array(tags), **arrays)
        env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
        env["CFHD_TEST_FRESH_CHILD"] = "1"
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "ref-child", src, dst], env=env, capture_output=True, text=True, timeout=900)
        assert run.returncode == 0 and "DECODED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
        got = np.load(dst)
        return {k: got[k] for k in got.files}


def ref_consistent_pairs(samples, w, h, tags):
    """[(RG48 picture, YU64 picture, words that differ per attempt)] of the reference decoder for every sample: the first pair among REF_ATTEMPTS decodes of each in
    which the YU64 picture is rgb_as_yuv_model of the RG48 picture with the sample's tag (the last count is 0), or its last decodes (the last count is not 0)."""
    got = _run_ref_child(samples, w, h, tags)
    return [(got["rg48_%d" % i], got["yu64_%d" % i], [int(c) for c in got["counts%d" % i]]) for i in range(len(samples))]


def ref_yu64_equal_to(samples, w, h, want):
    """[(the reference's YU64 picture, words that differ from want[i] per attempt)]: the first of REF_ATTEMPTS decodes of sample i that equals want[i], or the last."""
    got = _run_ref_child(samples, w, h, [0] * len(samples), want)
    return [(got["yu64_%d" % i], [int(c) for c in got["counts%d" % i]]) for i in range(len(samples))]


# ---- the expected contents of a device buffer
def elements(words, layout):
    """uint16 words [rows, n] in the element type of the layout: uint8 [rows, n * E]."""
    words = np.ascontiguousarray(words)
    if layout in (RGB_AS_YU64, RGB_AS_YUV422_U16): return words.view(np.uint8).reshape(words.shape[0], -1)
    f32 = words.astype(np.float32) * (np.float32(1) / np.float32(65535))
    assert f32.dtype == np.float32
    if layout == RGB_AS_YUV422_F32: return np.ascontiguousarray(f32).view(np.uint8).reshape(words.shape[0], -1)
    return np.ascontiguousarray(f32.astype(np.float16)).view(np.uint8).reshape(words.shape[0], -1)


def geometry(w, h, layout, padded):
    """(row bytes of the first plane or of the packed row, pitch, stride): the contiguous form -- packed: 4 w; planes: one row of an (N, 2 H W) tensor -- or a pitch
    with padding (+ 48 packed, + 64 planes: the plane pitch stays a multiple of 32) and a stride of + 4096."""
    if layout == RGB_AS_YU64:
        row = 4 * w
        pitch = ((row + 15) & ~15) + (48 if padded else 0)
        return row, pitch, h * pitch + (4096 if padded else 0)
    row = w * ELEMENT[layout]
    pitch = ((row + 31) & ~31) + (64 if padded else 0)
    return row, pitch, 2 * h * pitch + (4096 if padded else 0)


def smallest_stride(w, h, layout, pitch):
    if layout == RGB_AS_YU64: return pitch * (h - 1) + 4 * w
    return pitch * h + (pitch // 2) * (2 * h - 1) + w * ELEMENT[layout] // 2


def place(image, at, w, h, layout, pitch, item):
    """One picture -- (the RG48 picture, the tag of its sample) or ZERO -- at image[at:] in the layout."""
    if item is ZERO: y = np.zeros((h, w), np.uint16); cb = np.zeros((h, w // 2), np.uint16); cr = cb
    else: y, cb, cr = M.yuv_of_rg48(item[0], w, h, item[1])
    if layout == RGB_AS_YU64:
        packed = np.empty((h, w // 2, 4), np.uint16)
        packed[:, :, 0] = y[:, 0::2]; packed[:, :, 1] = cr; packed[:, :, 2] = y[:, 1::2]; packed[:, :, 3] = cb
        image[at: at + h * pitch].reshape(h, pitch)[:, : 4 * w] = packed.reshape(h, 2 * w).view(np.uint8)
        return
    E = ELEMENT[layout]
    image[at: at + h * pitch].reshape(h, pitch)[:, : w * E] = elements(y, layout)
    half = pitch // 2
    for k, plane in enumerate((cb, cr)):
        start = at + h * pitch + k * h * half
        image[start: start + h * half].reshape(h, half)[:, : (w // 2) * E] = elements(plane, layout)


class Delivery(DP.Delivery):
    """device_pictures.Delivery for the pictures of an RG48 batch of RGB samples in one of the four layouts.  The pictures handed to expect / check are
    (RG48 picture, tag), ZERO or None (untouched)."""
    def __init__(self, q, layout, padded, npictures):
        self.q, self.layout = q, layout
        self.row, self.pitch, self.stride = geometry(q.w, q.h, layout, padded)
        self.image = pattern(GUARD + npictures * self.stride + GUARD)
        self.mem = DeviceArray(self.image)

    def expect(self, pictures):
        for i, p in enumerate(pictures):
            if p is not None: place(self.image, GUARD + i * self.stride, self.q.w, self.q.h, self.layout, self.pitch, p)
        return self.image


def run_pass(q, samples, sizes=None, count=None): return DP.run_pass(q, samples, sizes, count)


def tagged(pictures, samples): return [(p, tag_of(s)) for p, s in zip(pictures, samples)]


# ---- 1. delivery equals the model on download_output of the same pass, and the reference's YU64 picture
# name: (kind of sample, w, h, samples in the batch and the pass)
DELIVERY_CASES = {
    "192x96-8": ("444", 192, 96, 8),                             # 12 groups of 16, 24 of 8: a partial wave
    "200x64-5": ("444", 200, 64, 5),                             # 25 groups of 8; 12 groups of 16 and four pairs behind them
    "72x40-3": ("444", 72, 40, 3),                               # the narrowest RGB frame the encoder takes: 4 groups of 16 and four pairs
    "504x24-2": ("444", 504, 24, 2),                             # more than one 62-block strip segment; 31 groups of 16 and four pairs
    "1040x24-2": ("444", 1040, 24, 2),                           # 130 groups of 8, 65 of 16: a lane's second and third trip along the row
    "rgba-192x96-8": ("4444", 192, 96, 8),                       # an RGBA 4:4:4:4 batch
}
DELIVERY_IDS = list(DELIVERY_CASES)


def check_delivery(name):
    """Every layout, into the contiguous geometry and into a padded pitch and stride, on one batch: the layout is switched between passes."""
    kind, w, h, n = DELIVERY_CASES[name]
    samples = samples_of(kind, w, h, n)
    reference = None
    q = DQ.Queue(samples[0], "RG48", FULL, n)
    L = lib()
    try:
        assert (q.w, q.h, q.row_bytes) == (w, h, 6 * w)
        seen = set()
        for layout in LAYOUTS:
            for padded in (False, True):
                what = "%s, %s, %s" % (name, LAYOUT_NAMES[layout], "padded pitch and stride" if padded else "the smallest pitch")
                d = Delivery(q, layout, padded, n)
                if not padded and layout == RGB_AS_YU64: assert d.pitch == 4 * w and d.stride == h * d.pitch
                if not padded and layout != RGB_AS_YU64 and d.row % 32 == 0: assert d.pitch == w * ELEMENT[layout] and d.stride == 2 * h * d.pitch      # a row of an (N, 2 H W) tensor
                if padded: assert d.pitch > d.row and d.stride > (h if layout == RGB_AS_YU64 else 2 * h) * d.pitch
                d.set()
                assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
                ret, status = run_pass(q, samples)
                assert ret == n and status == [0] * n, (what, ret, status, amd_last_error())
                want = q.pictures(n)
                assert len(set(p.tobytes() for p in want)) == n
                d.check(tagged(want, samples), what)
                models = [M.yu64_of_rg48(want[i], w, h, tag_of(samples[i])) for i in range(n)]
                seen |= {int(m.view(np.uint16).min()) for m in models} | {int(m.view(np.uint16).max()) for m in models}
                if have_ref() and layout in (RGB_AS_YU64, RGB_AS_YUV422_U16):
                    # the reference decoder's YU64 picture of each sample (asked once per case: the pictures of a pass are the same in every pass)
                    if reference is None: reference = ref_yu64_equal_to(samples, w, h, models)
                    for i in range(n):
                        assert np.array_equal(models[i], reference[i][0]), "%s: picture %d differs from the reference decoder's YU64 picture (words that differ, per attempt: %s)" % (what, i, reference[i][1])
        print("%s: the delivered words reach %d .. %d" % (name, min(seen), max(seen)))
    finally:
        q.close()


# ---- 2. a short pass touches nothing else; switching to PACKED, to NULL and back, the name under index 9 each time
def check_short_pass_and_switching(layout):
    w, h = SHAPE
    samples = samples_of("444", w, h)
    q = DQ.Queue(samples[0], "RG48", FULL, 8)
    L = lib()
    try:
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        d = Delivery(q, layout, True, 8); d.set()
        ret, status = run_pass(q, samples, count=3)
        assert (ret, status) == (3, [0] * 3)
        d.check(tagged(q.pictures(3), samples) + [None] * 5, "count = 3 of 8: rows, padding, gaps, the pictures behind the count, the guards")
        packed = DP.Delivery(q, PACKED, True, 8); packed.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        ret, status = run_pass(q, samples[5:8])
        assert (ret, status) == (3, [0] * 3)
        packed.check(q.pictures(3) + [None] * 5, "PACKED (the RG48 picture) behind an RGB_AS layout")
        d.check([None] * 8, "the YUV buffer while PACKED is set")
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        ret, status = run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check([None] * 8, "the YUV buffer after set_device_pictures(NULL)")
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        planar = DP.Delivery(q, DP.PLANAR_F16, False, 8); planar.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        ret, status = run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        planar.check(q.pictures(8), "PLANAR_F16 (R, G, B planes) on the same batch")
        d.set()
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
        ret, status = run_pass(q, samples)
        assert ret == 8 and status == [0] * 8
        d.check(tagged(q.pictures(8), samples), "count = 8 behind PACKED, NULL and PLANAR_F16")
    finally:
        q.close()


# ---- 3. a pass that mixes untagged samples and samples tagged 4
def golden():
    """(the reference-encoded 192 x 96 RG48 -> 4:4:4 sample made with flag bit 8, the reference decoder's YU64 picture of it: uint8 [96, 768])."""
    sample = open(GOLDEN_SAMPLE, "rb").read()
    return sample, np.load(GOLDEN_YU64)


def make_golden():
    """Writes the two files under tests/golden/ (needs oracle/_ref): frame 3 of the patched 192 x 96 frames, seed 41, through the reference's encoder with
    CFHD_ENCODING_FLAGS bit 8, and the reference decoder's YU64 picture of that sample."""
    w, h = SHAPE
    sample = samples_of("444", w, h, 4, FLAG_VIDEO_SYSTEMS, "ref", seed=41)[3]
    assert tag_of(sample) & 4
    rg48, yu64, counts = ref_consistent_pairs([sample], w, h, [tag_of(sample)])[0]
    assert counts[-1] == 0, counts
    for k in range(3): assert np.array_equal(ref_yu64_equal_to([sample], w, h, [yu64])[0][0], yu64)      # (... and it is the picture the reference gives again)
    open(GOLDEN_SAMPLE, "wb").write(sample); np.save(GOLDEN_YU64, yu64)
    print("%d byte sample, tag %d; picture %s" % (len(sample), tag_of(sample), yu64.shape))


MIXED_TAGGED = (1, 2, 5)                                        # the places of the tagged sample in the mixed pass: a run of two and a run of one


def mixed_pass():
    w, h = SHAPE
    plain = samples_of("444", w, h)
    sample, yu64 = golden()
    assert tag_of(plain[0]) & 4 == 0 and tag_of(sample) & 4 == 4
    samples = [sample if i in MIXED_TAGGED else plain[i] for i in range(8)]
    return plain, samples, yu64


def check_mixed_pass(layout):
    """The batch is prepared on an untagged sample; the tagged ones come back through the handle inside wait and are delivered by a launch of their own with the
    video-systems matrix: their pictures equal the reference's YU64 picture of the sample, word for word."""
    w, h = SHAPE
    plain, samples, yu64 = mixed_pass()
    q = DQ.Queue(plain[0], "RG48", FULL, 8)
    try:
        for padded in (False, True):
            d = Delivery(q, layout, padded, 8); d.set()
            ret, status = run_pass(q, samples)
            assert ret == 8 and status == [0] * 8, (ret, status, amd_last_error())
            want = q.pictures(8)
            d.check(tagged(want, samples), "the mixed pass, %s" % LAYOUT_NAMES[layout])
            for i in MIXED_TAGGED:
                assert np.array_equal(M.yu64_of_rg48(want[i], w, h, 4), yu64), "picture %d: the model on download_output differs from the reference's YU64 picture" % i
                assert not np.array_equal(M.yu64_of_rg48(want[i], w, h, 0), yu64), "the two matrices give the same picture: the test shows nothing"
            words = np.ascontiguousarray(yu64).view(np.uint16)
            assert words.max() == 65535 and words.min() == 0, "the video-systems picture does not saturate at both ends"
            if layout in (RGB_AS_YU64, RGB_AS_YUV422_U16):      # ... and the device buffer itself, without the model in between
                got = d.mem.read()
                for i in MIXED_TAGGED:
                    at = GUARD + i * d.stride
                    if layout == RGB_AS_YU64: assert np.array_equal(got[at: at + h * d.pitch].reshape(h, d.pitch)[:, : 4 * w], yu64)
                    else:
                        y, cb, cr = M.planes_of_yu64(yu64, w, h)
                        assert np.array_equal(got[at: at + h * d.pitch].reshape(h, d.pitch)[:, : 2 * w], y.view(np.uint8).reshape(h, 2 * w))
                        half = d.pitch // 2
                        for k, plane in enumerate((cb, cr)):
                            start = at + h * d.pitch + k * h * half
                            assert np.array_equal(got[start: start + h * half].reshape(h, half)[:, : w], plane.view(np.uint8).reshape(h, w))
    finally:
        q.close()


# ---- 4. verdicts: a sample that failed is zeros, its neighbours are intact
def check_failed_samples(layout):
    """Pass A: a sample cut in half and one with another frame width -- the parser's verdict is final, the launch of the pass writes zeros in their places.  Pass B: a
    damaged code stream -- every sample the parser passed goes through the handle inside wait and is delivered by launches there, zeros where the handle refused.
    Pass C: intact samples in the same buffer."""
    w, h = SHAPE
    intact = samples_of("444", w, h)
    q = DQ.Queue(intact[0], "RG48", FULL, 8)
    try:
        d = Delivery(q, layout, True, 8); d.set()
        for name, damage in (("A", {2: "cut in half", 6: "frame width"}), ("B", {3: "payload pattern"})):
            samples = list(intact); sizes = [len(s) for s in samples]
            for i, kind in damage.items(): samples[i], sizes[i] = DQ.damaged(kind, samples[i], None)
            res, _ = DQ.handle_pictures(samples, "RG48", FULL, sizes=sizes, first=intact[0])
            codes = [rc for rc, _ in res]
            print("pass %s: the handle answers %s" % (name, codes))
            assert codes.count(0) >= 6 and (name == "B" or (codes[2] and codes[6]))
            ret, status = run_pass(q, samples, sizes)
            assert status == codes and ret == codes.count(0), (status, codes)
            got = q.pictures(8)
            for i, rc in enumerate(codes):
                if rc: assert not got[i].any(), "picture %d of a sample that failed is not zero" % i
                else: assert np.array_equal(got[i], res[i][1]), "picture %d differs from the handle's" % i
            # (ZERO: every row byte of the picture 0 -- 0.0 in the float layouts --, and not the conversion of a black picture, whose luma is 4096)
            d.check([ZERO if rc else (got[i], tag_of(intact[i])) for i, rc in enumerate(codes)], "pass %s, %s" % (name, LAYOUT_NAMES[layout]))
        ret, status = run_pass(q, intact)
        assert ret == 8 and status == [0] * 8
        d.check(tagged(q.pictures(8), intact), "an intact pass behind the damaged ones")
    finally:
        q.close()


# ---- 5. the two submit paths, host delivery beside device delivery
def check_submit_paths(layout):
    w, h = SHAPE
    samples = samples_of("444", w, h)
    L = lib()
    q = DQ.Queue(samples[0], "RG48", FULL, 8)
    try:
        blob, offsets, sizes = DQ.scattered_blob(list(samples))
        d = Delivery(q, layout, True, 8); d.set()
        frame = q.row_bytes * q.h
        host = np.full(frame * 8, 9, np.uint8)
        assert q.submit(blob, offsets, sizes, host, frame, q.row_bytes) == 0, amd_last_error()
        assert q.wait(8) == (8, [0] * 8)
        want = q.pictures(8)
        for i in range(8): assert np.array_equal(host[i * frame: (i + 1) * frame], want[i]), "submit_host: the host picture %d beside device delivery is not the RG48 picture" % i
        d.check(tagged(want, samples), "submit_host, %s" % LAYOUT_NAMES[layout])
        d2 = Delivery(q, layout, False, 8); d2.set()
        owner, dptr = DQ.device_copy(blob)
        if dptr is None: dptr = owner.ptr
        assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, _sizes(offsets), _sizes(sizes), 8) == 0, amd_last_error()
        assert q.wait(8) == (8, [0] * 8)
        again = q.pictures(8)
        for i in range(8): assert np.array_equal(again[i], want[i])
        d2.check(tagged(again, samples), "submit_device, %s" % LAYOUT_NAMES[layout])
        d.check([None] * 8, "the first buffer while another is set")
        del owner
    finally:
        q.close()


# ---- 6. gates
def check_gates():
    w, h = SHAPE
    L = lib()
    rgb, rgba, yuv = samples_of("444", w, h), samples_of("4444", w, h), DQ.samples_of("422", w, h, "amd")
    import bayer_queue as BQ
    served = {"444": DQ.Queue(rgb[0], "RG48", FULL, 8), "4444": DQ.Queue(rgba[0], "RG48", FULL, 2)}
    unserved = {"422": DQ.Queue(yuv[0], "RG48", FULL, 2), "444-half": DQ.Queue(rgb[0], "RG48", HALF, 2), "groups": GQ.GroupQueue(GQ.group_stream("amd", w, h, 0)[0], "RG48", FULL, 2)}
    foreign = {"444-b64a": DQ.Queue(rgb[0], "b64a", FULL, 2), "422-YU64": DQ.Queue(yuv[0], "YU64", FULL, 2), "444-RG24": DQ.Queue(rgb[0], "RG24", FULL, 2), "bayer": BQ.Queue(BQ.samples_of(w, h, "amd")[0], 2)}
    try:
        q = served["444"]
        d = Delivery(q, RGB_AS_YUV422_F32, True, 8)
        p, stride, pitch = d.mem.ptr + GUARD, d.stride, d.pitch
        def refused(queue, ptr, s, pt, layout, what):
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, ptr, s, pt, layout) == -1, what
            text = amd_last_error()
            assert text and "decode queue" in text, "%s: refused without a text (%r)" % (what, text)
            return text
        def accepted(queue, ptr, s, pt, layout, what):
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, ptr, s, pt, layout) == 0, "%s: %s" % (what, amd_last_error())
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, None, 0, 0, 0) == 0
        # served where they belong
        for name, queue in served.items():
            for layout in LAYOUTS:
                assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, p, stride, pitch, layout) == 0, "%s, %s: %s" % (name, LAYOUT_NAMES[layout], amd_last_error())
                assert L.cfhd_amd_decode_batch_kernel_name(queue.b, 9) == DELIVER
            assert L.cfhd_amd_decode_batch_set_device_pictures(queue.b, None, 0, 0, 0) == 0
            assert L.cfhd_amd_decode_batch_kernel_name(queue.b, 9) == b"k_dec_deliver"
        # the RG48 batches they do not serve: one new text
        not_served = set(refused(queue, p, stride, pitch, layout, "%s on the %s batch" % (LAYOUT_NAMES[layout], name)) for name, queue in unserved.items() for layout in LAYOUTS)
        assert len(not_served) == 1, not_served
        text = next(iter(not_served))
        assert "RGB 4:4:4" in text and "RGBA 4:4:4:4" in text and "full" in text and "4:2:2 sample decodes to YU64 directly" in text, text
        # every batch whose output is not RG48: unknown, as before
        for name, queue in foreign.items():
            for layout in LAYOUTS: assert refused(queue, p, stride, pitch, layout, "%s on the %s batch" % (LAYOUT_NAMES[layout], name)) == PARENT_UNKNOWN
        # layouts 0 .. 14, -1 and 19 on the RG48 batches, served and unserved: what they answered before
        for name, queue in list(served.items()) + list(unserved.items()):
            for layout in (4, 5, 6, 11, 12, 13, 14, -1, 19): assert refused(queue, p, stride, pitch, layout, "layout %d on the %s batch" % (layout, name)) == PARENT_UNKNOWN
            for layout in (7, 8, 9, 10): assert refused(queue, p, stride, pitch, layout, "layout %d on the %s batch" % (layout, name)) == PARENT_YUV422
            for layout in (1, 2, 3): accepted(queue, p, 3 * queue.h * queue.w * 4, queue.w * 4, layout, "layout %d on the %s batch" % (layout, name))
            accepted(queue, p, queue.h * queue.row_bytes, queue.row_bytes, PACKED, "PACKED on the %s batch" % name)
            assert refused(queue, p, stride, queue.row_bytes - 16, PACKED, "a low pitch, packed, %s" % name) == PARENT_LOW_PITCH
            assert refused(queue, p, 16, queue.row_bytes, PACKED, "a low stride, packed, %s" % name) == PARENT_LOW_STRIDE
            assert refused(queue, p, stride, queue.w * 2 - 16, 1, "a low pitch, planar u16, %s" % name) == PARENT_LOW_PITCH
        for name in ("444-b64a", "444-RG24"):
            for layout in (1, 2, 3): assert refused(foreign[name], p, stride, pitch, layout, "layout %d on the %s batch" % (layout, name)) == PARENT_PLANAR
        assert refused(foreign["422-YU64"], p, stride, pitch, 7, "YUV422_U8 on a YU64 batch") == PARENT_U8_ON_YU64
        # the new refusals of the served batches: an odd width cannot be made (the encoders take no such frame); pitch and stride
        low_pitch_packed = refused(q, p, stride, 4 * w - 16, RGB_AS_YU64, "a pitch below 4 W")
        low_pitch_planes = set(refused(q, p, stride, w * ELEMENT[layout] - 32, layout, "a pitch below W x element size, %s" % LAYOUT_NAMES[layout]) for layout in LAYOUTS[1:])
        low_pitch_planes.add(refused(q, p, stride, -pitch, RGB_AS_YUV422_F32, "a negative pitch"))
        pitch_32 = set(refused(q, p, stride, pitch + 16, layout, "a plane pitch that is no multiple of 32, %s" % LAYOUT_NAMES[layout]) for layout in LAYOUTS[1:])
        low_stride_packed = refused(q, p, smallest_stride(w, h, RGB_AS_YU64, 4 * w) - 16, 4 * w, RGB_AS_YU64, "a stride below the rows")
        low_stride_planes = set(refused(q, p, smallest_stride(w, h, layout, pt) - 16, pt, layout, "a stride below the three planes, %s" % LAYOUT_NAMES[layout])
                                for layout, pt in ((RGB_AS_YUV422_U16, w * 2), (RGB_AS_YUV422_F16, pitch), (RGB_AS_YUV422_F32, w * 4)))
        off = set([refused(q, p + 8, stride, pitch, layout, "a pointer off 16") for layout in LAYOUTS] + [refused(q, p, stride + 8, pitch, RGB_AS_YU64, "a stride off 16"), refused(q, p, stride, pitch + 8, RGB_AS_YU64, "a pitch off 16")])
        assert off == {PARENT_OFF_16}
        for s in (low_pitch_planes, pitch_32, low_stride_planes): assert len(s) == 1, s
        new = {text, low_pitch_packed, low_stride_packed} | low_pitch_planes | pitch_32 | low_stride_planes
        parent = {PARENT_UNKNOWN, PARENT_PLANAR, PARENT_YUV422, PARENT_OFF_16, PARENT_LOW_PITCH, PARENT_LOW_STRIDE, PARENT_U8_ON_YU64}
        yu64 = foreign["422-YU64"]
        parent |= set([refused(yu64, p, stride, 64, 8, "a low pitch, 4:2:2 planes"), refused(yu64, p, 32, pitch - pitch % 32, 8, "a low stride, 4:2:2 planes"), refused(yu64, p, stride, pitch + 16, 8, "a pitch off 32, 4:2:2 planes")])
        assert len(new) == 6 and not (new & parent), "the texts of the new refusals are distinct from each other and from the existing ones: %s" % sorted(new)
        # the smallest pitch and stride are served
        accepted(q, p, smallest_stride(w, h, RGB_AS_YU64, 4 * w), 4 * w, RGB_AS_YU64, "the smallest packed geometry")
        for layout in LAYOUTS[1:]: accepted(q, p, smallest_stride(w, h, layout, w * ELEMENT[layout]), w * ELEMENT[layout], layout, "the smallest geometry, %s" % LAYOUT_NAMES[layout])
        # a refusal leaves the layout that was set in place, and nothing was launched
        d.set()
        refused(q, p, stride, w * 4 - 32, RGB_AS_YUV422_F32, "a pitch below the f32 luma row, again")
        d.check([None] * 8, "behind refused calls")
        # a pass in flight refuses
        blob, offsets, sizes = DQ.pack(rgb)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        try:
            assert "flight" in refused(q, p, stride, pitch, RGB_AS_YUV422_F32, "a pass in flight")
        finally:
            ret, status = q.wait(8)
        assert ret == 8 and status == [0] * 8
        d.check(tagged(q.pictures(8), rgb), "the pass the refused call was made in")
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == DELIVER
    finally:
        for x in list(served.values()) + list(unserved.values()) + list(foreign.values()): x.close()


# ---- 7. the kernel's time and name (hardware)
def check_kernel_times():
    w, h = SHAPE
    L = lib()
    samples = samples_of("444", w, h)
    q = DQ.Queue(samples[0], "RG48", FULL, 8)
    try:
        assert L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        d = Delivery(q, RGB_AS_YUV422_F16, False, 8); d.set()
        assert run_pass(q, samples) == (8, [0] * 8)
        ms, name = L.cfhd_amd_decode_batch_kernel_ms(q.b, 9), L.cfhd_amd_decode_batch_kernel_name(q.b, 9)
        print("k_dec_deliver_rgb_as_yuv, 8 pictures of %d x %d: %.4f ms" % (w, h, ms))
        assert ms > 0 and name == DELIVER, (ms, name)
        packed = DP.Delivery(q, PACKED, False, 8); packed.set()
        assert run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) > 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
        assert L.cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        assert run_pass(q, samples) == (8, [0] * 8)
        assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 9) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 9) == b"k_dec_deliver"
    finally:
        q.close()


# ---- 8. a torch tensor (hardware)
def check_torch(torch):
    """Delivery into one row of an (N, 2 H W) tensor through its data_ptr(), viewed as Y (H, W) and CbCr (2, H, W / 2), against the model."""
    w, h = SHAPE
    samples = samples_of("444", w, h)
    for layout, dtype in ((RGB_AS_YUV422_U16, torch.int16), (RGB_AS_YUV422_F16, torch.float16), (RGB_AS_YUV422_F32, torch.float32)):
        q = DQ.Queue(samples[0], "RG48", FULL, 8)
        try:
            E = ELEMENT[layout]
            t = torch.zeros((8, 2 * h * w), dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            assert lib().cfhd_amd_decode_batch_set_device_pictures(q.b, t.data_ptr(), 2 * h * w * E, w * E, layout) == 0, amd_last_error()
            assert run_pass(q, samples) == (8, [0] * 8)
            want = q.pictures(8)
            y, cbcr = t[:, : h * w].view(8, h, w), t[:, h * w:].view(8, 2, h, w // 2)
            torch.cuda.synchronize()
            gy, gc = y.cpu().numpy(), cbcr.cpu().numpy()
            for i in range(8):
                my, mcb, mcr = M.yuv_of_rg48(want[i], w, h, tag_of(samples[i]))
                assert np.array_equal(np.ascontiguousarray(gy[i]).view(np.uint8).reshape(h, w * E), elements(my, layout)), "%s: Y of picture %d" % (LAYOUT_NAMES[layout], i)
                assert np.array_equal(np.ascontiguousarray(gc[i, 0]).view(np.uint8).reshape(h, w // 2 * E), elements(mcb, layout)), "%s: Cb of picture %d" % (LAYOUT_NAMES[layout], i)
                assert np.array_equal(np.ascontiguousarray(gc[i, 1]).view(np.uint8).reshape(h, w // 2 * E), elements(mcr, layout)), "%s: Cr of picture %d" % (LAYOUT_NAMES[layout], i)
        finally:
            q.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["make-golden"]: make_golden()
    elif sys.argv[1:2] == ["ref-child"]: _ref_child(sys.argv[2], sys.argv[3])
