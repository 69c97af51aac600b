"""Every encoded format at every quality word, both ways: the helpers and test bodies shared by tests/test_gpu_quality_matrix.py (hardware) and
tests/test_quality_matrix_emulated.py (the same functions inside cfhd_testlib.emulated_product(), on a subset).

The quality word steers, per format, the subband tables (cfhd_tables.cpp derive_subband_tables / derive_quantization: luma or chroma tables, the precision-12 branch with
its chroma gain from the RGB-quality bits, the Bayer pin, the interlaced adjustments, the midpoint prequant with its wrap above 8, the low-frequency divisors, the bit-rate
limiter, the FILMSCAN2/3 feedback) and through them what the kernels meet: the 16-bit wrap of |x| + midpoint, the divisor <= 1 bypass and the 24-bit multiply of quantize /
pk_quantize, the HL band's midpoint, the decoder's value * quant tables, and the run lengths of nearly empty (LOW) or dense (FILMSCAN3) bands.

What is checked against what:
  encode    three frames through one CFHD_EncodeSample handle (the feedback state moves) against the reference encoder driven the same way: equal sizes, equal bytes
            after mask_volatile_metadata, frame by frame.
  decode    the REFERENCE's sample of frame 2 through CFHD_DecodeSample at full and at half resolution; every output with the acceptance of its existing test in
            tests/test_gpu_parity.py: 8-bit 4:2:2 inside the dither interval of the oracle's exact reconstruction (_check_decode), every 16-bit output word for word
            the oracle's inverse, the reference decoder beside it as a witness (cfhd_testlib.reference_leg).
  strips    the register-strip kernels forced on their smallest geometries (CFHD_AMD_FORWARD / _INVERSE / _PLANES = strip), the kernel names asserted.
  host      the limiter's size gate, quality switches on one handle and on the pool, and the quality words that are rewritten or refused (make_params).
Test infrastructure only: nothing here is a product path."""
import ctypes, os
import numpy as np
from cfhd_testlib import *

W, H = 192, 96                      # the tiled kernels run here, and the emulator manages it
INTERLACED = 1
KEYING = 5 | 0x04000000             # CFHD_ENCODING_QUALITY_KEYING: FILMSCAN2 with RGB quality 2 (chroma gain 4 in the precision-12 branch)
DETAIL = lambda d: 4 | d << 17      # FILMSCAN1 with the detail bits: midpoint prequant 2 + d, wrapping to 0 above 8 (d = 7)
ENCODED = {"422": ENCODED_YUV422, "444": ENCODED_RGB444, "4444": ENCODED_RGBA4444, "bayer": ENCODED_BAYER}
# route: (input pixel format, encoded format, encoding flags)
ROUTES = {"%s-%s%s" % (f, e, "i" if fl else ""): (f, e, fl) for f, e, fl in [
    ("YUY2", "422", 0), ("2vuy", "422", INTERLACED), ("v210", "422", 0), ("YU64", "422", 0), ("RG24", "422", 0), ("BGRa", "422", 0), ("RG48", "422", 0), ("a214", "422", 0),
    ("RG48", "444", 0), ("RG24", "444", 0), ("r210", "444", 0), ("b64a", "444", 0), ("RG64", "444", 0), ("b64a", "4444", 0), ("BGRA", "4444", 0),
    ("BYR4", "bayer", 0), ("BYR5", "bayer", 0)]}
ENCODE_WORDS = [1, 2, 3, 5, 6, KEYING, 4 | 0x02000000, DETAIL(1), DETAIL(3), DETAIL(6), DETAIL(7), 10]
# 336 x 252: odd lowpass widths (42 -> 21 chroma columns at level 3) and pad rows 252 -> 256
ENCODE_CASES = [(r, W, H, q) for r in ROUTES for q in ENCODE_WORDS] + [(r, 336, 252, q) for r in ("YUY2-422", "RG48-444") for q in ENCODE_WORDS]
DECODE_CASES = [(r, q) for r, (f, e, fl) in ROUTES.items() for q in [1, 3, 6, DETAIL(3)] + ([KEYING] if e in ("444", "4444") else [])]
# the emulator is slow: every route at 1 and 6, every word on one route per encoded format
MAIN_ROUTES = ("YUY2-422", "RG48-444", "b64a-4444", "BYR4-bayer")
EMULATED_ENCODE_CASES = [c for c in ENCODE_CASES if c[1] == W and (c[3] in (1, 6) or c[0] in MAIN_ROUTES)]
EMULATED_DECODE_CASES = [c for c in DECODE_CASES if c[1] in (1, 6) or c[0] in MAIN_ROUTES]
# the smallest geometries of test_yuv422_strip_kernels_equal_reference, test_interlaced_strip_..., test_packed16_strip_... and test_bayer_strip_... (tests/test_gpu_parity.py)
STRIP_GEOMETRY = {"YUY2-422": (2304, 72), "2vuy-422i": (2048, 120), "RG48-444": (504, 242), "b64a-4444": (136, 120), "BYR4-bayer": (1008, 244)}
STRIP_KERNELS = {"YUY2-422": (b"k_fwd_yuv422_strip_blocks", b"k_inv_yuv422_strip_blocks"), "2vuy-422i": (b"k_fwd_frame_yuv422_strip", b"k_inv_frame_yuv422_strip_blocks"),
                 "RG48-444": (b"k_fwd_packed16_strip", b"k_inv_packed16_strip"), "b64a-4444": (b"k_fwd_packed16_strip", b"k_inv_packed16_strip"), "BYR4-bayer": (b"k_fwd_bayer_strip", None)}
STRIP_CASES = [(r, q) for r in STRIP_GEOMETRY for q in [1, 3, DETAIL(3), DETAIL(7)] + ([KEYING] if ROUTES[r][1] in ("444", "4444") else [])]
# (FILMSCAN2, FILMSCAN3, and KEYING -- FILMSCAN2 with the RGB-quality bits -- on the RGB routes: the words no batch takes)
STRIP_HANDLE_CASES = [(r, q) for r in STRIP_GEOMETRY for q in [5, 6] + ([KEYING] if ROUTES[r][1] in ("444", "4444") else [])]
# (the handle keeps the level-1 coefficients for its host writer: the same strip kernel, writing dense bands beside its block lists)
STRIP_HANDLE_KERNELS = {r: k[0] for r, k in STRIP_KERNELS.items()}; STRIP_HANDLE_KERNELS["YUY2-422"] = b"k_fwd_yuv422_strip_blocks_dense"
EMULATED_STRIP_CASES = [("b64a-4444", 1), ("b64a-4444", DETAIL(7)), ("RG48-444", KEYING)]
EMULATED_STRIP_HANDLE_CASES = [("b64a-4444", 6), ("YUY2-422", 5)]
# above 1920 pixels or above 1080 rows the bit-rate limiter is off; 1920 x 64 beside them.  (144 x 1088: the size gate refuses 64 x 1088 -- NARROW below -- and 144 pixels
# is the narrowest 4:2:2 frame above 1080 rows that it takes.)
LIMITER_CASES = [(w, h, q) for w, h in ((1936, 64), (144, 1088), (1920, 64)) for q in (1, 2, 3)]
# (route, widest refused width, narrowest width taken): frames with level-3 bands of 8 columns or fewer in some channel are refused (make_params)
NARROW = [("YUY2-422", 128, 144), ("2vuy-422i", 128, 144), ("v210-422", 96, 144), ("RG48-422", 128, 144), ("RG48-444", 64, 72), ("b64a-4444", 64, 72), ("BYR4-bayer", 128, 144)]
RAW_STORABLE = ("v210", "r210", "DPX0", "AB10", "AR10", "RG30", "BYR4", "BYR5")      # the inputs the reference can store raw (encoder.c:1972-1975)
UNCOMPRESSED_WORDS = (4 | 4 << 8, 4 | 16 << 8)
case_id = lambda v: "0x%x" % v if isinstance(v, int) and v > 0xffff else str(v)      # (pytest asks per value)


def _fourcc(name): return fourcc(name)
def raw_size(fmt, pitch): return H * W * 3 // 2 if fmt in ("BYR4", "BYR5") else H * pitch      # (the mosaics are stored packed to 12 bits: encoder.c:7699-7737)


_frames, _refs = {}, {}


def route_frames(route, w, h, n=3):
    """n distinct frames of the route's input (computed once, shared, read-only) and their pitch."""
    key = (route, w, h, n)
    if key not in _frames:
        import avid_frames, test_input_routes_emulated as R
        fmt, _, flags = ROUTES[route] if route in ROUTES else (route, None, 0)
        if fmt == "a214": fr, pitch, _ = avid_frames.frames(fmt, w, h, n)
        else:
            made = [R._frame("AB10" if fmt == "RG30" else fmt, w, h, 7 + i) for i in range(n)]
            fr, pitch = [f for f, _ in made], made[0][1]
            for i, f in enumerate(fr):
                if flags & INTERLACED: v = f.reshape(h, pitch); v[1::2] = np.roll(v[1::2], 8 * (i + 1), axis=1)      # the second field a little later
                f.setflags(write=False)
        _frames[key] = (list(fr), pitch)
    return _frames[key]


def ref_samples(route, w, h, quality, n=3):
    """The reference encoder's samples of the route's frames through one handle (computed once per route, geometry and word)."""
    key = (route, w, h, quality, n)
    if key not in _refs:
        fmt, enc, flags = ROUTES[route]
        frames, pitch = route_frames(route, w, h, n)
        if quality & 0x1f00: frames = [f.copy() for f in frames]      # (in its uncompressed mode the reference writes into the caller's frame)
        _refs[key] = ref_encode_frames(frames, pitch, w, h, pixfmt=_fourcc(fmt), encoded=ENCODED[enc], quality=quality, flags=flags)
    return _refs[key]


def assert_samples_equal(mine, refs, what=""):
    assert len(mine) == len(refs)
    for i, (a, b) in enumerate(zip(mine, refs)):
        assert len(a) == len(b), "%sframe %d: %d bytes vs reference %d" % (what, i, len(a), len(b))
        ma, mb = mask_volatile_metadata(a), mask_volatile_metadata(b)
        if ma != mb:
            diff = [k for k in range(len(ma)) if ma[k] != mb[k]]
            raise AssertionError("%sframe %d differs from the reference in %d bytes, first at %d of %d" % (what, i, len(diff), diff[0], len(ma)))


# ------------------------------------------------------------------------------------------
# 1. encode
# ------------------------------------------------------------------------------------------
def check_encode(route, w, h, quality):
    fmt, enc, flags = ROUTES[route]
    frames, pitch = route_frames(route, w, h)
    refs = ref_samples(route, w, h, quality)
    mine = amd_encode_frames(frames, pitch, w, h, _fourcc(fmt), encoded=ENCODED[enc], quality=quality, flags=flags)
    assert_samples_equal(mine, refs)


# ------------------------------------------------------------------------------------------
# 2. decode
# ------------------------------------------------------------------------------------------
def _rows(buf, pitch, dtype, rows, cols):
    return np.frombuffer(buf.tobytes(), dtype).reshape(-1, pitch // np.dtype(dtype).itemsize)[:rows, :cols]


def _exact16(sample, name, want, dtype, half, w, h, leg_what, agree=None, attempts=6):
    """One 16- or 32-bit output: the product's picture word for word `want`; the reference decoder's picture of the same sample as a witness (agree(reference's rows,
    mine): the comparison of the existing test of that output, plain equality by default)."""
    got, gpitch, aw, ah = amd_decode_sample(sample, _fourcc(name), resolution=2 if half else 1)
    assert (aw, ah) == ((w // 2, h // 2) if half else (w, h)), (name, half, aw, ah)
    mine = _rows(got, gpitch, dtype, ah, want.shape[1])
    assert mine.shape == want[:ah].shape and np.array_equal(mine, want[:ah]), "%s%s: %d words differ from the exact reconstruction" % (name, " at half resolution" if half else "", (mine != want[:ah]).sum())
    if leg_what is None: return mine
    def leg():
        dec, dpitch = ref_decode_sample(sample, w, h, _fourcc(name), resolution=2 if half else 1)
        img = _rows(dec, dpitch, dtype, ah, want.shape[1])
        if agree: return agree(img, mine)
        return np.array_equal(img, mine) or "%d words differ" % (img != mine).sum()
    reference_leg(leg, attempts, leg_what)
    return mine


def _interval8(sample, w, h, pixfmt, interlaced):
    """_check_decode's interval for a sample whose source was not an 8-bit 4:2:2 frame: every byte the oracle's exact reconstruction with dither 0 or with dither 1, the
    dither balanced, the reference's own picture inside the interval.  (What it leaves out is _check_decode's PSNR against the source frame: there is none in this format.)"""
    out, pitch, aw, ah = amd_decode_sample(sample, pixfmt)
    assert (aw, ah) == (w, h)
    img = out.reshape(ah, pitch)[:, : w * 2]
    plan = Plan(w, h, pixkind=2 if pixfmt == PIX_2VUY else 1, progressive=0 if interlaced else 1)
    coeffs = oracle_decode_pyramid(sample, plan)
    inverse = oracle_inverse_interlaced_yuv422 if interlaced else oracle_inverse_yuv422
    lo = inverse(plan, coeffs, 0, uyvy=int(pixfmt == PIX_2VUY))[:h]; hi = inverse(plan, coeffs, 1, uyvy=int(pixfmt == PIX_2VUY))[:h]
    ok = (img == lo) | (img == hi)
    assert ok.all(), "%d of %d bytes are outside the dither interval of the exact reconstruction" % ((~ok).sum(), ok.size)
    if (lo != hi).sum() > 1000:
        frac = (img[lo != hi] == hi[lo != hi]).mean()
        assert 0.35 < frac < 0.65, "dither is not balanced: %.3f" % frac
    def leg():
        rout, rpitch = ref_decode_sample(sample, w, h, pixfmt)
        rimg = rout.reshape(h, rpitch)[:, : w * 2]
        return bool(((rimg == lo) | (rimg == hi)).all()) or "the reference's own output leaves the dither interval"
    reference_leg(leg, 3, "4:2:2 -> 8-bit 4:2:2")


def check_decode(route, quality):
    """The reference's sample of frame 2 at this word, decoded to every output the existing tests pin for its encoded format, at full and at half resolution."""
    from test_gpu_parity import _check_decode
    fmt, enc, flags = ROUTES[route]
    w, h = W, H
    frames, pitch = route_frames(route, w, h)
    sample = ref_samples(route, w, h, quality)[2]
    if enc == "422":
        interlaced = bool(flags & INTERLACED)
        out8 = PIX_2VUY if fmt == "2vuy" else PIX_YUY2
        if fmt in ("YUY2", "2vuy"): _check_decode(sample, np.asarray(frames[2]), w, h, out8, interlaced=interlaced)
        else: _interval8(sample, w, h, out8, interlaced)
        plan8 = Plan(w, h, pixkind=2 if out8 == PIX_2VUY else 1, progressive=0 if interlaced else 1)
        want = oracle_half_resolution(plan8, oracle_decode_pyramid(sample, plan8), int(out8 == PIX_2VUY))
        _exact16(sample, "2vuy" if out8 == PIX_2VUY else "YUY2", want, np.uint8, True, w, h, "interlaced 4:2:2 at half resolution" if interlaced else "4:2:2 at half resolution", attempts=4)
        if interlaced: return      # (the 16-bit outputs of interlaced samples: tests/test_gpu_interlaced_rgb.py; YU64 / v210 are refused at full resolution)
        plan = Plan(w, h, pixkind=PIXKIND["YU64"])
        deq = oracle_decode_pyramid(sample, plan)
        _exact16(sample, "YU64", oracle_inverse_yu64(plan, deq), np.uint16, False, w, h, "4:2:2 -> YU64")
        _exact16(sample, "YU64", oracle_half_resolution_yu64(plan, deq), np.uint16, True, w, h, "4:2:2 -> YU64 at half resolution")
        _exact16(sample, "v210", oracle_inverse_v210(plan, deq, w), np.uint32, False, w, h, "4:2:2 -> v210", attempts=3)
        _exact16(sample, "v210", oracle_half_resolution_v210(plan, deq), np.uint32, True, w, h, "4:2:2 -> v210 at half resolution")
        for name in ("RG48", "b64a"):
            plan = Plan(w, h, pixkind=PIXKIND[name], enc=ENC["422"])
            deq = oracle_decode_pyramid(sample, plan)
            _exact16(sample, name, oracle_inverse_rgb16_of_yuv422(plan, deq, name == "b64a", 2), np.uint16, False, w, h, "4:2:2 -> %s" % name, attempts=4)
            _exact16(sample, name, oracle_half_resolution_rgb16_of_yuv422(plan, deq, name == "b64a", 2), np.uint16, True, w, h, "4:2:2 -> %s at half resolution" % name, attempts=4)
    elif enc == "444":
        plan = Plan(w, h, pixkind=PIXKIND["RG48"], enc=ENC["444"])
        deq = oracle_decode_pyramid(sample, plan)
        _exact16(sample, "RG48", oracle_inverse_rgb48(plan, deq), np.uint16, False, w, h, "RGB 4:4:4 -> RG48", attempts=3)
        half = oracle_half_resolution16(plan, deq, False)[: h // 2]
        _exact16(sample, "RG48", half, np.uint16, True, w, h, "RG48 at half resolution", agree=lambda img, mine: half16_equal(img, half, None, 3), attempts=4)
        _exact16(sample, "b64a", oracle_half_resolution_rgb(plan, deq, "b64a"), np.uint16, True, w, h, "RGB 4:4:4 -> b64a at half resolution")
        plan = Plan(w, h, pixkind=PIXKIND["b64a"], enc=ENC["444"])
        _exact16(sample, "b64a", oracle_inverse_b64a_of_rgb444(plan, oracle_decode_pyramid(sample, plan)), np.uint16, False, w, h, "RGB 4:4:4 -> b64a")
    elif enc == "4444":
        plan = Plan(w, h, pixkind=PIXKIND["b64a"], enc=ENC["4444"])
        deq = oracle_decode_pyramid(sample, plan)
        exact = oracle_inverse_rgb48(plan, deq, b64a=True)[:h]; raw = oracle_inverse_rgb48(plan, deq, b64a=False)[:h]
        def alpha_race(img, mine):          # colour words exact, alpha rows expanded or -- the reference's race on alpha_Companded, bayer.c:13871 / :16034 -- left companded
            colour = all(np.array_equal(img[:, k::4], exact[:, k::4]) for k in (1, 2, 3))
            rows = (img[:, 0::4] == exact[:, 0::4]).all(axis=1) | (img[:, 0::4] == raw[:, 3::4]).all(axis=1)
            return bool(colour and rows.all())
        _exact16(sample, "b64a", exact, np.uint16, False, w, h, "RGBA 4:4:4:4 -> b64a", agree=alpha_race, attempts=3)
        half = oracle_half_resolution16(plan, deq, True)[: h // 2]; half_raw = oracle_half_resolution16(plan, deq, True, expand_alpha=False)[: h // 2]
        _exact16(sample, "b64a", half, np.uint16, True, w, h, "b64a at half resolution", agree=lambda img, mine: half16_equal(img, half, half_raw, 4), attempts=4)
        _exact16(sample, "RG48", oracle_inverse_rgb48(plan, deq)[:h].reshape(h, w, 4)[:, :, :3].reshape(h, w * 3), np.uint16, False, w, h, "RGBA 4:4:4:4 -> RG48")
        _exact16(sample, "RG48", oracle_half_resolution16(plan, deq), np.uint16, True, w, h, None)      # (no witness: the reference's answer on this route depends on its process's history, cfhd_testlib.ref_decode_sample_fresh_process)
    else:
        plan = Plan(w, h, pixkind=PIXKIND["BYR4"], enc=ENC["bayer"])
        _exact16(sample, "BYR4", oracle_inverse_byr4(plan, oracle_decode_pyramid(sample, plan))[:h, :w], np.uint16, False, w, h, "Bayer -> BYR4")


# ------------------------------------------------------------------------------------------
# 3. strip kernels
# ------------------------------------------------------------------------------------------
class strip_shapes:
    """CFHD_AMD_FORWARD / _INVERSE / _PLANES = strip (read at every launch), put back on the way out."""
    KEYS = ("CFHD_AMD_FORWARD", "CFHD_AMD_INVERSE", "CFHD_AMD_PLANES")
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.KEYS}
        for k in self.KEYS: os.environ[k] = "strip"
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def quantizer_is_static(route, w, h, quality):
    """The product's own answer: front_end_params' static_quantizer (quantizer_is_static, cfhd_api_gather.h) through cfhd_amd_quantizer_is_static."""
    fmt, enc, flags = ROUTES[route]
    L = product()
    L.cfhd_amd_quantizer_is_static.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
    rc = L.cfhd_amd_quantizer_is_static(w, h, _fourcc(fmt), ENCODED[enc], flags, quality)
    assert rc in (0, 1), "front_end_params refused %s %d x %d 0x%x" % (route, w, h, quality)
    return bool(rc)


def _check_strip_pictures(route, w, h, sample, picture):
    """picture: the bytes of one decoded frame at its natural pitch."""
    fmt, enc, flags = ROUTES[route]
    if enc == "422":
        uyvy = int(fmt == "2vuy"); interlaced = bool(flags & INTERLACED)
        plan = Plan(w, h, pixkind=2 if uyvy else 1, progressive=0 if interlaced else 1)
        deq = oracle_decode_pyramid(sample, plan)
        inverse = oracle_inverse_interlaced_yuv422 if interlaced else oracle_inverse_yuv422
        lo, hi = inverse(plan, deq, 0, uyvy=uyvy)[:h], inverse(plan, deq, 1, uyvy=uyvy)[:h]
        img = picture.reshape(h, w * 2)
        ok = (img == lo) | (img == hi)
        assert ok.all(), "%d bytes outside the dither interval" % (~ok).sum()
    else:
        b64a = fmt == "b64a"
        plan = Plan(w, h, pixkind=PIXKIND[fmt], enc=ENC[enc])
        want = oracle_inverse_rgb48(plan, oracle_decode_pyramid(sample, plan), b64a=b64a)[:h]
        got = np.frombuffer(picture.tobytes(), np.uint16).reshape(h, -1)
        assert np.array_equal(got, want), "%d words differ from the exact reconstruction" % (got != want).sum()


def check_strip(route, quality):
    """Two frames through a batch with the strip kernels forced: the kernel names, the samples against the reference encoder's, the pictures as in check_decode.  A word
    the batch front end refuses must be one whose quantizer moves with the size of the previous sample (rate feedback: the frames of a batch are encoded side by side)."""
    import group_batches as GB
    L = GB.lib()
    fmt, enc, flags = ROUTES[route]
    w, h = STRIP_GEOMETRY[route]
    frames, pitch = route_frames(route, w, h, 2)
    mode = 1 if enc == "bayer" else 0           # (Bayer batches are encode only; the sample is decoded through CFHD_DecodeSample below)
    with strip_shapes():
        b = L.cfhd_amd_batch_create_ex(w, h, _fourcc(fmt), ENCODED[enc], flags, quality, 2, 2, mode)
        static = quantizer_is_static(route, w, h, quality)
        if not b:
            assert not static, "cfhd_amd_batch_create_ex refused a word whose quantizer is static (%s)" % amd_last_error()
            return False
        try:
            assert static, "cfhd_amd_batch_create_ex took a word whose quantizer moves with the previous sample"
            for i, f in enumerate(frames): assert L.cfhd_amd_batch_upload(b, i, np.asarray(f).ctypes.data_as(ctypes.c_void_p), pitch) == 0, amd_last_error()
            fwd, inv = STRIP_KERNELS[route]
            assert L.cfhd_amd_batch_kernel_name(b, 0) == fwd, L.cfhd_amd_batch_kernel_name(b, 0)
            if inv: assert L.cfhd_amd_batch_kernel_name(b, 3) == inv, L.cfhd_amd_batch_kernel_name(b, 3)
            if route == "YUY2-422":         # level-2 luma planes of 72 blocks: levels 2 and 3 as plane strips too, as test_yuv422_strip_kernels_equal_reference asserts
                assert [L.cfhd_amd_batch_kernel_name(b, k) for k in (1, 2, 4, 5)] == [b"k_fwd_plane_strip", b"k_fwd_plane_strip", b"k_inv_plane_strip", b"k_inv_plane_strip"]
            assert L.cfhd_amd_batch_roundtrip(b) > 0, amd_last_error()
            refs = ref_samples(route, w, h, quality, 2)
            mine = []
            for i in range(2):
                p = ctypes.c_void_p(); sz = ctypes.c_size_t()
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                mine.append(ctypes.string_at(p, sz.value))
            assert_samples_equal(mine, refs)
            for i in range(2 if mode == 0 else 0):
                out = np.zeros(h * pitch, np.uint8)
                assert L.cfhd_amd_batch_download_output(b, i, out.ctypes.data_as(ctypes.c_void_p), pitch) == 0, amd_last_error()
                _check_strip_pictures(route, w, h, mine[i], out)
        finally:
            L.cfhd_amd_batch_destroy(b)
        if enc == "bayer":
            plan = Plan(w, h, pixkind=PIXKIND["BYR4"], enc=ENC["bayer"])
            _exact16(refs[1], "BYR4", oracle_inverse_byr4(plan, oracle_decode_pyramid(refs[1], plan))[:h, :w], np.uint16, False, w, h, "Bayer -> BYR4")
    return True


def handle_encode(steps, w, h, fmt, enc, flags, L=None, kernel=None):
    """One CFHD_EncodeSample handle prepared with the quality of each step in turn -- the second and later prepares take the 'just changing quality' path of
    CFHD_PrepareToEncode (same geometry, formats and flags) --: the samples of all steps.  steps: [(quality, frames, pitch)].  L: the library (the product by default).
    kernel: the level-1 kernel the handle must report before its first frame."""
    L = L or product()
    e = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(e), None) == 0
    out = []
    try:
        for k, (quality, frames, pitch) in enumerate(steps):
            rc = L.CFHD_PrepareToEncode(e, w, h, _fourcc(fmt), ENCODED[enc], flags, quality)
            assert rc == 0, "CFHD_PrepareToEncode(0x%x) -> %d" % (quality, rc)
            if kernel and k == 0:
                L.cfhd_amd_encoder_kernel_name.restype = ctypes.c_char_p; L.cfhd_amd_encoder_kernel_name.argtypes = [ctypes.c_void_p]
                assert L.cfhd_amd_encoder_kernel_name(e) == kernel, L.cfhd_amd_encoder_kernel_name(e)
            for f in frames:
                rc = L.CFHD_EncodeSample(e, np.asarray(f).ctypes.data_as(ctypes.c_void_p), pitch)
                assert rc == 0, "CFHD_EncodeSample -> %d" % rc
                p = ctypes.c_void_p(); n = ctypes.c_size_t()
                assert L.CFHD_GetSampleData(e, ctypes.byref(p), ctypes.byref(n)) == 0
                out.append(ctypes.string_at(p, n.value))
    finally:
        L.CFHD_CloseEncoder(e)
    return out


def check_strip_handle(route, quality):
    """The feedback qualities (FILMSCAN2 / FILMSCAN3), which no batch takes, through the C ABI's handle with the strip kernels forced: the handle launches through the same
    EncodeBatch and honours the same variables; cfhd_amd_encoder_kernel_name says which level-1 kernel it runs."""
    fmt, enc, flags = ROUTES[route]
    w, h = STRIP_GEOMETRY[route]
    frames, pitch = route_frames(route, w, h, 2)
    assert not quantizer_is_static(route, w, h, quality)
    with strip_shapes():
        mine = handle_encode([(quality, frames, pitch)], w, h, fmt, enc, flags, kernel=STRIP_HANDLE_KERNELS[route])
    assert_samples_equal(mine, ref_samples(route, w, h, quality, 2))


# ------------------------------------------------------------------------------------------
# 4. limiter boundary, quality switches
# ------------------------------------------------------------------------------------------
def check_limiter_geometry(w, h, quality):
    """YUY2 at LOW / MEDIUM / HIGH, four frames through one handle on either side of the limiter's size bound (cfhd_tables.cpp bitrate_limiter_applies), bytes against the
    reference's.  Frames this small stay far below the 110 .. 150 Mbit/s at which the limiter moves, so these cases run the kernels at the geometries and show that
    nothing else changes at the bound; the bound itself is pinned on the host by check_limiter_size_bound."""
    frames = [synth_yuy2(w, h, 40 + i)[0] for i in range(4)]
    refs = ref_encode_frames(frames, w * 2, w, h, quality=quality)
    assert_samples_equal(amd_encode_frames(frames, w * 2, w, h, quality=quality), refs)


def check_limiter_size_bound():
    """bitrate_limiter_applies' size bound, on the host (the hooks library's cfhd_amd_quant_sequence: the tables of frame 2 after a previous sample of 1 MB, 250 Mbit/s at
    the limiter's 30 fps and beyond every limit): at 1920 x 1080 the tables of MEDIUM / HIGH move, at 1936 x 1080 and at 1920 x 1088 they stay; RGB 4:4:4 and four channels never move.  (LOW has
    no coarser table to move to -- its limiter table is its own -- and the limiter's further scaling lands on the subbands of the two-frame group that an intra frame
    does not code: its tables stay at every size.)"""
    def moves(w, h, fmt, enc, quality):
        nch = Plan(w, h, pixkind=PIXKIND[fmt], enc=ENC[enc]).num_channels
        sizes = (ctypes.c_longlong * 2)(1000000, 0); out = (ctypes.c_int * (2 * 9 * nch))()
        assert hooks().cfhd_amd_quant_sequence(w, h, PIXKIND[fmt], ENC[enc], quality, 1, sizes, 2, out) == 2 * 9 * nch
        return list(out[: 9 * nch]) != list(out[9 * nch:])
    for quality in (1, 2, 3):
        assert moves(1920, 1080, "YUY2", "422", quality) == (quality != 1), quality
        assert not moves(1936, 1080, "YUY2", "422", quality) and not moves(1920, 1088, "YUY2", "422", quality), quality
        assert not moves(1920, 1080, "RG48", "444", quality) and not moves(1920, 1080, "b64a", "4444", quality), quality
    assert not moves(1920, 1080, "YUY2", "422", 4)
    # ... and the product's own answer (quantizer_is_static through cfhd_amd_quantizer_is_static), which is what keeps such words out of the batches
    L = product()
    L.cfhd_amd_quantizer_is_static.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
    for quality in (1, 2, 3):
        assert [L.cfhd_amd_quantizer_is_static(w, h, PIX_YUY2, ENCODED_YUV422, 0, quality) for w, h in ((1920, 1080), (1936, 1080), (1920, 1088))] == [int(quality == 1), 1, 1], quality


SWITCHES = (4, 1, 6, 4)


def check_quality_switches_on_one_handle(route="YUY2-422"):
    """One handle re-prepared in mid-stream, FILMSCAN1 -> LOW -> FILMSCAN3 -> FILMSCAN1 with two frames at each, against the reference driven the same way: the 'just
    changing quality' path of CFHD_PrepareToEncode, which keeps the frame counter, the size of the last sample and the limiter state seeded by the first prepare."""
    fmt, enc, flags = ROUTES[route]
    frames, pitch = route_frames(route, W, H, 8)
    steps = [(q, frames[2 * k: 2 * k + 2], pitch) for k, q in enumerate(SWITCHES)]
    assert_samples_equal(handle_encode(steps, W, H, fmt, enc, flags), handle_encode(steps, W, H, fmt, enc, flags, L=ref()))


def pool_encode(L, steps, w, h, fmt, enc, flags):
    """The samples of a pool of one worker whose quality is changed between submissions (CFHD_PrepareEncoderPool on a started pool), in submission order."""
    pool = ctypes.c_void_p()
    assert L.CFHD_CreateEncoderPool(ctypes.byref(pool), 1, 4, None) == 0
    out = []; number = 0
    try:
        for k, (quality, frames, pitch) in enumerate(steps):
            assert L.CFHD_PrepareEncoderPool(pool, w, h, _fourcc(fmt), ENCODED[enc], flags, quality) == 0, "CFHD_PrepareEncoderPool(0x%x)" % quality
            if k == 0: assert L.CFHD_StartEncoderPool(pool) == 0
            for f in frames:
                number += 1
                assert L.CFHD_EncodeAsyncSample(pool, number, np.asarray(f).ctypes.data_as(ctypes.c_void_p), pitch, None) == 0
                num = ctypes.c_uint32(); sb = ctypes.c_void_p()
                assert L.CFHD_WaitForSample(pool, ctypes.byref(num), ctypes.byref(sb)) == 0 and num.value == number
                p = ctypes.c_void_p(); n = ctypes.c_size_t()
                assert L.CFHD_GetEncodedSample(sb, ctypes.byref(p), ctypes.byref(n)) == 0
                out.append(ctypes.string_at(p, n.value))
                assert L.CFHD_ReleaseSampleBuffer(pool, sb) == 0
    finally:
        L.CFHD_StopEncoderPool(pool); L.CFHD_ReleaseEncoderPool(pool)
    return out


def check_quality_switches_on_the_pool(route="YUY2-422"):
    """The same sequence through an encoder pool of one worker, each frame collected before the next is submitted, against the reference's pool driven the same way."""
    from test_gpu_parity import normalise_frame_counters
    fmt, enc, flags = ROUTES[route]
    frames, pitch = route_frames(route, W, H, 8)
    steps = [(q, frames[2 * k: 2 * k + 2], pitch) for k, q in enumerate(SWITCHES)]
    mine = [normalise_frame_counters(s) for s in pool_encode(product(), steps, W, H, fmt, enc, flags)]
    refs = [normalise_frame_counters(s) for s in pool_encode(ref(), steps, W, H, fmt, enc, flags)]
    assert_samples_equal(mine, refs)


# ------------------------------------------------------------------------------------------
# 5. quality words that are rewritten or refused
# ------------------------------------------------------------------------------------------
REWRITE_ROUTES = ("YUY2-422", "RG48-444", "b64a-4444", "RG24-422")


def check_uncompressed_bits_on_other_inputs(route, quality):
    """The uncompressed bits (0x1f00) on an input the reference cannot store raw: FILMSCAN2's tables without rate feedback, and (word & ~0x1fff) | 6 in the header's
    QUALITY_L (encoder.c:2022-2029) -- bytes equal the reference's, on a fresh handle and through the 'just changing quality' path."""
    fmt, enc, flags = ROUTES[route]
    frames, pitch = route_frames(route, W, H)
    refs = ref_samples(route, W, H, quality)
    mine = amd_encode_frames(frames, pitch, W, H, _fourcc(fmt), encoded=ENCODED[enc], quality=quality, flags=flags)
    assert_samples_equal(mine, refs)
    steps = [(4, frames[:1], pitch), (quality, frames[1:], pitch)]
    assert_samples_equal(handle_encode(steps, W, H, fmt, enc, flags), handle_encode([(q, [f.copy() for f in fr], p) for q, fr, p in steps], W, H, fmt, enc, flags, L=ref()), "after a quality change: ")
    if route == "YUY2-422":       # ... and as the new word of a running pool (a word without format marks: the reference's pool hands its workers the caller's word as it is)
        from test_gpu_parity import normalise_frame_counters
        mine, refs = [[normalise_frame_counters(s) for s in pool_encode(L, steps, W, H, fmt, enc, flags)] for L in (product(), ref())]
        assert_samples_equal(mine, refs, "pool after a quality change: ")


def _prepare_rc(L, w, h, fmt, enc, flags, quality):
    e = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(e), None) == 0
    try: return L.CFHD_PrepareToEncode(e, w, h, _fourcc(fmt), ENCODED[enc], flags, quality)
    finally: L.CFHD_CloseEncoder(e)


RAW_ENCODED = {"v210": "422", "BYR4": "bayer", "BYR5": "bayer"}      # (the 10-bit RGB words: "444")


def check_uncompressed_mode_is_refused(fmt):
    """The uncompressed bits on an input the reference can store raw: CFHD_ERROR_BADFORMAT from the handle (fresh and on a quality change), the pool and
    cfhd_amd_batch_create_ex -- the uncompressed mode is not built.  Witness: the reference answers the same call with at least one sample of the raw size."""
    import group_batches as GB
    L = GB.lib()
    enc = RAW_ENCODED.get(fmt, "444")
    frames, pitch = route_frames(fmt, W, H)
    for quality in UNCOMPRESSED_WORDS:
        assert _prepare_rc(L, W, H, fmt, enc, 0, quality) == 3, "CFHD_PrepareToEncode took 0x%x from %s" % (quality, fmt)
        e = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(e), None) == 0
        assert L.CFHD_PrepareToEncode(e, W, H, _fourcc(fmt), ENCODED[enc], 0, 4) == 0
        assert L.CFHD_PrepareToEncode(e, W, H, _fourcc(fmt), ENCODED[enc], 0, quality) == 3, "the quality change took 0x%x from %s" % (quality, fmt)
        assert L.CFHD_EncodeSample(e, np.asarray(frames[0]).ctypes.data_as(ctypes.c_void_p), pitch) == 0      # (the handle keeps what it was prepared with)
        L.CFHD_CloseEncoder(e)
        pool = ctypes.c_void_p(); assert L.CFHD_CreateEncoderPool(ctypes.byref(pool), 1, 4, None) == 0
        assert L.CFHD_PrepareEncoderPool(pool, W, H, _fourcc(fmt), ENCODED[enc], 0, quality) == 3
        L.CFHD_ReleaseEncoderPool(pool)
        b = L.cfhd_amd_batch_create_ex(W, H, _fourcc(fmt), ENCODED[enc], 0, quality, 2, 1, 1)
        if b: L.cfhd_amd_batch_destroy(b)
        assert not b, "cfhd_amd_batch_create_ex took 0x%x from %s" % (quality, fmt)
        refs = ref_encode_frames([f.copy() for f in frames], pitch, W, H, pixfmt=_fourcc(fmt), encoded=ENCODED[enc], quality=quality)
        # (4 << 8 asks for a quarter of the frames, drawn by a lottery seeded with the frame's first bytes; 16 << 8 for all of them)
        if quality == 4 | 16 << 8: assert all(len(s) >= raw_size(fmt, pitch) for s in refs), "the reference stored no frame of %s raw at 0x%x: %s" % (fmt, quality, [len(s) for s in refs])


def reference_uncompressed_sample(fmt):
    enc = RAW_ENCODED.get(fmt, "444")
    frames, pitch = route_frames(fmt, W, H)
    refs = ref_encode_frames([f.copy() for f in frames], pitch, W, H, pixfmt=_fourcc(fmt), encoded=ENCODED[enc], quality=4 | 16 << 8)
    return max(refs, key=len), pitch


def check_uncompressed_samples_are_refused(fmt, out):
    """The reference's uncompressed sample of a v210 / r210 / BYR4 frame: refused with CFHD_ERROR_BADFORMAT and a text in cfhd_amd_last_error() -- by CFHD_PrepareToDecode
    when the bytes it is shown reach the UNCOMPRESS chunk tag, by CFHD_DecodeSample (picture zeroed) on a handle prepared with a compressed sample of the same route."""
    L = product()
    enc = RAW_ENCODED.get(fmt, "444")
    sample, pitch = reference_uncompressed_sample(fmt)
    assert len(sample) >= raw_size(fmt, pitch)
    frames, _ = route_frames(fmt, W, H)
    good = ref_encode_frames(frames[:1], pitch, W, H, pixfmt=_fourcc(fmt), encoded=ENCODED[enc])[0]
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
        sb = ctypes.create_string_buffer(sample, len(sample))
        gb = ctypes.create_string_buffer(good, len(good))
        assert L.CFHD_PrepareToDecode(dec, 0, 0, _fourcc(out), 1, 0, sb, len(sample), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 3
        assert "uncompressed" in amd_last_error(), amd_last_error()
        assert L.CFHD_PrepareToDecode(dec, 0, 0, _fourcc(out), 1, 0, gb, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
        p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
        picture = np.full(p.value * ah.value, 7, np.uint8)
        assert L.CFHD_DecodeSample(dec, sb, len(sample), picture.ctypes.data_as(ctypes.c_void_p), p.value) == 3
        assert "uncompressed" in amd_last_error(), amd_last_error()
        rowbytes = {"v210": (W // 6) * 16, "RG48": W * 6, "BYR4": W * 2}[out]
        assert not picture.reshape(ah.value, p.value)[:, :rowbytes].any(), "the refused picture is not zeroed"
        # the handle still decodes the compressed sample
        assert L.CFHD_DecodeSample(dec, gb, len(good), picture.ctypes.data_as(ctypes.c_void_p), p.value) == 0, amd_last_error()
        assert picture.any()
    finally:
        L.CFHD_CloseDecoder(dec)


def check_narrow_frames_are_refused(route, refused, taken):
    """Frames so narrow that a channel's level-3 bands are 8 columns or fewer: the reference's horizontal filter leaves other values in column 0 of its horizontal
    highpass bands there than the transform computes at every other width (64 x 96 YUY2 at FILMSCAN1: 6 604 bytes, where the kernels and the oracle come to 6 540).  Not
    restated, so refused -- CFHD_ERROR_BADFORMAT from the handle and the pool, NULL from cfhd_amd_batch_create_ex -- rather than encoded to other bytes; the narrowest
    width taken still gives the reference's bytes.  Witness: the reference takes the refused width."""
    import group_batches as GB
    L = GB.lib()
    fmt, enc, flags = ROUTES[route]
    assert _prepare_rc(L, refused, H, fmt, enc, flags, 4) == 3, "CFHD_PrepareToEncode took %s at %d pixels" % (route, refused)
    assert _prepare_rc(ref(), refused, H, fmt, enc, flags, 4) == 0
    pool = ctypes.c_void_p(); assert L.CFHD_CreateEncoderPool(ctypes.byref(pool), 1, 4, None) == 0
    assert L.CFHD_PrepareEncoderPool(pool, refused, H, _fourcc(fmt), ENCODED[enc], flags, 4) == 3
    L.CFHD_ReleaseEncoderPool(pool)
    b = L.cfhd_amd_batch_create_ex(refused, H, _fourcc(fmt), ENCODED[enc], flags, 4, 2, 1, 1)
    if b: L.cfhd_amd_batch_destroy(b)
    assert not b, "cfhd_amd_batch_create_ex took %s at %d pixels" % (route, refused)
    frames, pitch = route_frames(route, taken, H, 2)
    mine = amd_encode_frames(frames, pitch, taken, H, _fourcc(fmt), encoded=ENCODED[enc], flags=flags)
    assert_samples_equal(mine, ref_encode_frames(frames, pitch, taken, H, pixfmt=_fourcc(fmt), encoded=ENCODED[enc], flags=flags))


def check_fixed_quality_is_refused():
    """A quality word whose low byte is 0 (CFHD_ENCODING_QUALITY_FIXED: the reference derives its tables from a bit rate, QuantizationSetRate, which is not built) is
    refused with CFHD_ERROR_BADFORMAT on every route -- never again taken and answered with other bytes than the reference's."""
    import group_batches as GB
    L = GB.lib()
    for route, (fmt, enc, flags) in ROUTES.items():
        for quality in (0, 0x04000000, 3 << 17, 0x100):
            assert _prepare_rc(L, W, H, fmt, enc, flags, quality) == 3, "%s took the quality word 0x%x" % (route, quality)
    e = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(e), None) == 0
    assert L.CFHD_PrepareToEncode(e, W, H, PIX_YUY2, ENCODED_YUV422, 0, 4) == 0
    assert L.CFHD_PrepareToEncode(e, W, H, PIX_YUY2, ENCODED_YUV422, 0, 0) == 3              # the quality change
    L.CFHD_CloseEncoder(e)
    pool = ctypes.c_void_p(); assert L.CFHD_CreateEncoderPool(ctypes.byref(pool), 1, 4, None) == 0
    assert L.CFHD_PrepareEncoderPool(pool, W, H, PIX_YUY2, ENCODED_YUV422, 0, 0) == 3
    L.CFHD_ReleaseEncoderPool(pool)
    b = L.cfhd_amd_batch_create_ex(W, H, PIX_YUY2, ENCODED_YUV422, 0, 0, 2, 1, 1)
    if b: L.cfhd_amd_batch_destroy(b)
    assert not b
    # witness: the reference takes the word and writes samples
    frames, pitch = route_frames("YUY2-422", W, H)
    assert all(len(s) > 1000 for s in ref_encode_frames(frames, pitch, W, H, quality=0))
