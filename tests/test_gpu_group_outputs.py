"""Two-frame groups decoded through CFHD_DecodeSample to every output an intra 4:2:2 sample of the same scan decodes to: YU64, v210, RG24, BGRA, BGRa, RG48, b64a at
full resolution (interlaced groups: RG48, b64a, BGRA, BGRa through the 16-bit rows of the inverse frame transform) and every output at half resolution.  Both frames of
two consecutive groups equal tests/group_outputs_model.py -- pinned on the reference's group decoder by test_group_outputs_model_vs_ref.py -- word for word / byte for
byte (RG24: inside the interval of its 15-bit dither, both ends about equally often), with the GPU entropy stage and with the host coder; the reference decoder runs
beside it once per route as a witness.  Then the gates: what stays refused at CFHD_PrepareToDecode and at CFHD_DecodeSample."""
import ctypes, os
import numpy as np
import pytest
from cfhd_testlib import *
import group_outputs_model as M

INTERLACED = 1
MATRIX_601 = 4          # (the flag that makes the reference encoder tag the samples 601)
BADFORMAT = 3           # CFHD_ERROR_BADFORMAT
BAD_RESOLUTION = 11     # CFHD_ERROR_BAD_RESOLUTION

# (w, h, fmt, interlaced, flicker, flags): 320x240; a display height that is no multiple of 8 and odd chroma lowpass widths (336x252, 720x486); a v210 width whose half is
# whole six-pixel groups too (384); 1080p; interlaced groups of test_gop._interlaced_frames, with and without flicker; both colour matrices
CASES = [(320, 240, "YUY2", 0, 0, 0), (336, 252, "YUY2", 0, 0, MATRIX_601), (384, 96, "YUY2", 0, 0, MATRIX_601), (720, 486, "2vuy", 0, 0, 0),
         (336, 252, "YUY2", 1, 1, 0), (720, 486, "2vuy", 1, 0, MATRIX_601), (1920, 1080, "YUY2", 0, 0, 0), (1920, 1080, "YUY2", 1, 0, MATRIX_601)]
_witnessed = set()


def group_stream(w, h, fmt, interlaced, flicker, flags):
    """Reference-encoded stream: sequence header, group, P-frame header, group, P-frame header."""
    import test_gop
    frames = test_gop._interlaced_frames(w, h, 4, fourcc(fmt), bool(flicker)) if interlaced else test_gop._frames(w, h, 4, fourcc(fmt))
    samples = ref_encode_frames(frames, w * 2, w, h, pixfmt=fourcc(fmt), flags=ENCODING_FLAGS_2FRAME_GOP | interlaced | flags)
    gp = GopPlan(w, h, pixkind=PIXKIND[fmt], interlaced=interlaced)
    gp.source_frames, gp.source_fmt = frames, fmt          # (the RG24 acceptance measures the PSNR against the source)
    return samples, gp


def source_rgb24(gp, k, rows, color_space):
    """Source frame k of the stream as RG24 bytes (B, G, R, bottom row first, `rows` rows), through the computer-systems-range matrix of the decode (709: color_space 2,
    601: 1) in floating point: the common yardstick of the RG24 acceptance's PSNR comparison."""
    w = gp.width
    px = np.asarray(gp.source_frames[k]).reshape(-1)[: rows * w * 2].reshape(rows, w // 2, 4).astype(np.float64)
    if gp.source_fmt == "2vuy": cb, y0, cr, y1 = (px[:, :, i] for i in range(4))
    else: y0, cb, y1, cr = (px[:, :, i] for i in range(4))
    rv, gu, gv, bu = (1.596, 0.392, 0.813, 2.017) if color_space == 1 else (1.793, 0.213, 0.533, 2.112)
    out = np.zeros((rows, w // 2, 2, 3))
    for j, y in enumerate((y0, y1)):
        yy = 1.164 * (y - 16)
        out[:, :, j, 2] = yy + rv * (cr - 128); out[:, :, j, 1] = yy - gu * (cb - 128) - gv * (cr - 128); out[:, :, j, 0] = yy + bu * (cb - 128)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8).reshape(rows, 3 * w)[::-1]


def names_of(w, interlaced, half):
    names = (M.HALF_INTERLACED if interlaced else M.HALF) if half else (M.FULL_INTERLACED if interlaced else M.FULL_PROGRESSIVE)
    return [n for n in names if M.served(n, w, half)]


def decode_stream(samples, name, half, dec=None, prepare_on=1):
    """The product's pictures of every sample (None for the sequence header) through one handle prepared on samples[prepare_on]; returns (pictures, aw, ah, pitch)."""
    L = product()
    own = dec is None
    if own:
        dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
        first = samples[prepare_on]
        sb = ctypes.create_string_buffer(first, len(first))
        rc = L.CFHD_PrepareToDecode(dec, 0, 0, fourcc(name), 2 if half else 1, 0, sb, min(512, len(first)), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af))
        assert rc == 0, "CFHD_PrepareToDecode -> %d" % rc
        p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
        outs = []
        for k, s in enumerate(samples):
            sb = ctypes.create_string_buffer(s, len(s)); out = np.full(p.value * ah.value, 7, np.uint8)
            assert L.CFHD_DecodeSample(dec, sb, len(s), out.ctypes.data_as(ctypes.c_void_p), p.value) == 0, (k, amd_last_error())
            outs.append(None if len(s) <= 64 and k == 0 else out)
        return outs, aw.value, ah.value, p.value
    finally:
        if own: L.CFHD_CloseDecoder(dec)


def rg24_in_interval(img, lo_hi, src, share=(0.45, 0.55)):
    """The acceptance of the intra RG24-of-4:2:2 gate (test_gpu_parity.test_yuv422_decode_to_rg24_lies_in_the_reference_interval): every byte between the model's results for
    the dither values 0 and 32767, both ends about equally often, and the PSNR against the source (src: source_rgb24) between the PSNRs of the two ends, to 0.1 dB."""
    lo, hi = lo_hi
    ok = (img >= lo) & (img <= hi)
    if not ok.all(): return "%d bytes outside the interval" % (~ok).sum()
    differ = lo != hi
    frac = (img[differ] == hi[differ]).mean()
    if not share[0] < frac < share[1]: return "share of the upper end %.3f" % frac
    db = lambda x: 10 * np.log10(255.0 ** 2 / np.mean((x.astype(np.float64) - src) ** 2))
    mine, ends = db(img), (db(lo), db(hi))
    return True if min(ends) - 0.1 < mine < max(ends) + 0.1 else "PSNR %.2f dB outside %.2f .. %.2f" % (mine, min(ends), max(ends))


def ref_group_outputs(samples, name, half):
    """The reference's pictures of a group stream in output `name`, driven as cfhd_testlib.ref_decode_group_frames drives it (prepared on the first group sample, each
    group sample decoded until two calls agree to the dither bit, then the P-frame sample); the raw rows, to be cropped by the output's own pitch.  Returns
    ([(frame 0, frame 1) per group], aw, ah, pitch)."""
    groups = [k for k, s in enumerate(samples) if len(s) > 64]
    d = RefDecoder(samples[groups[0]], fourcc(name), 2 if half else 1, 1)
    def dec(s):
        sb = ctypes.create_string_buffer(s, len(s)); out = np.zeros(d.pitch * d.height + 64, np.uint8)
        assert d.decode(sb, len(s), out) == 0
        return out[: d.pitch * d.height].copy()
    got = []
    try:
        for k in groups:
            prev = dec(samples[k]); f0 = dec(samples[k])
            for _ in range(6):
                if (np.abs(f0.astype(np.int16) - prev) <= 1).all(): break
                prev = f0; f0 = dec(samples[k])
            f1 = dec(samples[k + 1]) if k + 1 < len(samples) and len(samples[k + 1]) <= 64 else None
            got.append((f0, f1))
        return got, d.width, d.height, d.pitch
    finally:
        d.close()


def check_stream(samples, gp, name, half, color_space, witness=True):
    """Both frames of both groups equal the model; one reference witness per route (output, resolution, scan)."""
    w = gp.width
    outs, aw, ah, pitch = decode_stream(samples, name, half)
    rows = 2 * ah if half else ah
    assert (aw, ah) == ((w // 2, gp.height // 2) if half else (w, gp.height))          # (prepared on the group sample: its display height)
    views = {}
    for g in range(2):
        want = M.model_decode_group(samples[2 * g + 1], gp, name, rows, color_space, half)
        for f in range(2):
            k = 2 * g + 1 + f
            if k >= len(outs): continue
            img = M.view_output(outs[k], pitch, aw, ah, name)
            src = source_rgb24(gp, 2 * g + f, rows, color_space if f == 0 else 2) if name == "RG24" and not half else None      # (frame 1: 709, the model says why)
            if name == "RG24" and not half:
                verdict = rg24_in_interval(img, want[f], src)
                assert verdict is True, "%s group %d frame %d: %s" % (name, g, f, verdict)
            else:
                assert np.array_equal(img, want[f]), "%s%s group %d frame %d: %d values differ from the model" % (name, " (half)" if half else "", g, f, (img != want[f]).sum())
            views[(g, f)] = (img, want[f], src)
    route = (name, half, gp.interlaced)
    if not witness or route in _witnessed or name == "BGRa" and gp.interlaced: return    # (the reference's own interlaced BGRa is not the picture: test_interlaced_rgb_model_vs_ref)
    _witnessed.add(route)
    def leg():
        got, raw, rah, rpitch = ref_group_outputs(samples, name, half)
        if (raw, rah) != (aw, ah): return "reference reports %dx%d" % (raw, rah)
        for (g, f), (img, want, src) in views.items():
            r = got[g][f]
            if r is None: continue
            r = M.view_output(r, rpitch, aw, ah, name)
            verdict = rg24_in_interval(r, want, src, (0.4, 0.6)) if name == "RG24" and not half else (np.array_equal(r, img) or "%d values differ" % (r != img).sum())
            if verdict is not True: return "group %d frame %d: %s" % (g, f, verdict)
        return True
    reference_leg(leg, 2, "two-frame groups -> %s%s%s" % (name, " at half resolution" if half else "", " (interlaced)" if gp.interlaced else ""))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("w,h,fmt,interlaced,flicker,flags", CASES)
def test_group_outputs_equal_model(w, h, fmt, interlaced, flicker, flags, half):
    samples, gp = group_stream(w, h, fmt, interlaced, flicker, flags)
    for name in names_of(w, interlaced, half):
        check_stream(samples, gp, name, bool(half), 1 if flags & MATRIX_601 else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,interlaced,flicker,flags", [(336, 252, "YUY2", 0, 0, MATRIX_601), (336, 252, "YUY2", 1, 1, 0)])
def test_group_outputs_with_host_entropy(w, h, fmt, interlaced, flicker, flags):
    """CFHD_AMD_ENTROPY=host: the host coder gives the lowpass band the same bias of the requested output (odd chroma lowpass widths: 21 columns)."""
    samples, gp = group_stream(w, h, fmt, interlaced, flicker, flags)
    old = os.environ.get("CFHD_AMD_ENTROPY")
    os.environ["CFHD_AMD_ENTROPY"] = "host"
    try:
        for half in (False, True):
            for name in names_of(w, interlaced, half):
                check_stream(samples, gp, name, half, 1 if flags & MATRIX_601 else 2, witness=False)
    finally:
        if old is None: os.environ.pop("CFHD_AMD_ENTROPY")
        else: os.environ["CFHD_AMD_ENTROPY"] = old


@pytest.mark.gpu
def test_interlaced_group_rows16_one_column_kernel():
    """CFHD_AMD_INVERSE=tile: the interlaced 16-bit rows through k_inv_frame_yuv422_rows16_col, the same words."""
    samples, gp = group_stream(336, 252, "YUY2", 1, 1, 0)
    old = os.environ.get("CFHD_AMD_INVERSE")
    os.environ["CFHD_AMD_INVERSE"] = "tile"
    try:
        for name in ("RG48", "BGRA"): check_stream(samples, gp, name, False, 2, witness=False)
    finally:
        if old is None: os.environ.pop("CFHD_AMD_INVERSE")
        else: os.environ["CFHD_AMD_INVERSE"] = old


@pytest.mark.gpu
def test_one_handle_reprepared_across_outputs_and_resolutions():
    """One handle, prepared on the sequence header: YUY2, then BGRA, then half-resolution YU64, then YUY2 again.  The sizes are the sequence header's (coded height;
    halved at half resolution); the YUY2 bytes of the last pass equal a fresh handle's (both draw the dither of the same call count: the counter is the handle's, so
    the second handle, which is never prepared for another output, decodes the stream as often)."""
    w, h = 336, 252
    samples, gp = group_stream(w, h, "YUY2", 0, 0, 0)
    H = (h + 7) // 8 * 8
    L = product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    fresh = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(fresh), None) == 0
    try:
        passes = [("YUY2", False), ("BGRA", False), ("YU64", True), ("YUY2", False)]
        for i, (name, half) in enumerate(passes):
            outs, aw, ah, pitch = decode_stream(samples, name, half, dec=dec, prepare_on=0)
            assert (aw, ah) == ((w // 2, H // 2) if half else (w, H))
            if name != "YUY2":
                want = M.model_decode_group(samples[1], gp, name, H, 2, half)
                assert np.array_equal(M.view_output(outs[1], pitch, aw, ah, name), want[0]), name
                assert np.array_equal(M.view_output(outs[2], pitch, aw, ah, name), want[1]), name
            # the fresh handle: prepared for YUY2 each time, so that its call counter keeps pace with the reused handle's
            fouts, _, _, _ = decode_stream(samples, "YUY2", False, dec=fresh, prepare_on=0)
        for k in range(1, len(samples)):
            assert np.array_equal(outs[k], fouts[k]), "sample %d: the re-prepared handle's YUY2 differs from a fresh handle's" % k
    finally:
        L.CFHD_CloseDecoder(dec); L.CFHD_CloseDecoder(fresh)


@pytest.mark.gpu
def test_group_prepare_gates():
    """Refused at CFHD_PrepareToDecode, as for intra 4:2:2 samples: the 10-bit RGB words (BADFORMAT) and quarter resolution (BAD_RESOLUTION); BGRA at half resolution
    where the half width is no multiple of 16, v210 where the width is no whole six-pixel groups."""
    samples, _ = group_stream(336, 252, "YUY2", 0, 0, 0)
    L = product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
        for s in samples[:2]:
            sb = ctypes.create_string_buffer(s, len(s))
            prep = lambda name, res: L.CFHD_PrepareToDecode(dec, 0, 0, fourcc(name), res, 0, sb, min(512, len(s)), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af))
            for name in ("r210", "DPX0", "AB10", "AR10"):
                assert prep(name, 1) == BADFORMAT and prep(name, 2) == BADFORMAT, name
            assert prep("YUY2", 3) == BAD_RESOLUTION and prep("BGRA", 3) == BAD_RESOLUTION
            assert prep("BGRA", 2) == BADFORMAT                     # (168 half columns)
            assert prep("BGRA", 1) == 0 and prep("v210", 1) == 0 and prep("v210", 2) == 0
        samples320, _ = group_stream(320, 240, "YUY2", 0, 0, 0)
        sb = ctypes.create_string_buffer(samples320[1], len(samples320[1]))
        assert L.CFHD_PrepareToDecode(dec, 0, 0, fourcc("v210"), 1, 0, sb, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == BADFORMAT
    finally:
        L.CFHD_CloseDecoder(dec)


REFUSALS = [("YU64", 0, 384), ("v210", 0, 384), ("RG24", 0, 384), ("RG24", 1, 384), ("BGRA", 0, 96), ("BGRa", 0, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,half,w", REFUSALS)
def test_interlaced_group_refusals_then_next_sample(name, half, w):
    """YU64 / v210 / RG24 of an interlaced group at full resolution (RG24 at half resolution too), and BGRA / BGRa below 128 pixels at full resolution (the width rule
    of the 16-bit rows), as for intra samples: CFHD_DecodeSample answers BADFORMAT with a zeroed picture, the P-frame sample behind it as well (no picture).  The same
    handle then decodes the next sample -- a progressive group, which serves these outputs -- to the model."""
    h = 96
    inter, _ = group_stream(w, h, "YUY2", 1, 0, 0)
    prog, gp = group_stream(w, h, "YUY2", 0, 0, 0)
    L = product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
        sb = ctypes.create_string_buffer(inter[1], len(inter[1]))
        assert L.CFHD_PrepareToDecode(dec, 0, 0, fourcc(name), 2 if half else 1, 0, sb, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
        p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
        for s in inter[1:3]:
            out = np.ones(p.value * ah.value, np.uint8)
            sb = ctypes.create_string_buffer(s, len(s))
            assert L.CFHD_DecodeSample(dec, sb, len(s), out.ctypes.data_as(ctypes.c_void_p), p.value) != 0
            assert not out.any()
        sb = ctypes.create_string_buffer(inter[1], len(inter[1]))
        assert L.CFHD_DecodeSample(dec, sb, len(inter[1]), np.ones(p.value * ah.value, np.uint8).ctypes.data_as(ctypes.c_void_p), p.value) == BADFORMAT
        rows = 2 * ah.value if half else ah.value
        want = M.model_decode_group(prog[1], gp, name, rows, 2, bool(half))
        for f, s in enumerate(prog[1:3]):
            out = np.zeros(p.value * ah.value, np.uint8)
            sb = ctypes.create_string_buffer(s, len(s))
            assert L.CFHD_DecodeSample(dec, sb, len(s), out.ctypes.data_as(ctypes.c_void_p), p.value) == 0, amd_last_error()
            img = M.view_output(out, p.value, aw.value, ah.value, name)
            if name == "RG24" and not half:
                verdict = rg24_in_interval(img, want[f], source_rgb24(gp, f, rows, 2))
                assert verdict is True, "frame %d: %s" % (f, verdict)
            else: assert np.array_equal(img, want[f]), "frame %d: %d values differ from the model" % (f, (img != want[f]).sum())
    finally:
        L.CFHD_CloseDecoder(dec)
