"""The hostile pictures of tests/hostile_pictures.py against the reference on the CPU: for every legal case of tests/test_gpu_hostile.py the reference encoder's sample
equals the oracle's transform + the host writer (masked), and the reference decoder's picture lies in the oracle's dither interval -- so the GPU tests may hold the
product to the oracle on these pictures.  Legality (`legal_for_reference`) is asserted on the oracle's prediction BEFORE the reference sees a picture: it overruns its
own sample buffer on the others."""
import numpy as np
import pytest
from cfhd_testlib import *
import hostile_pictures as H

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")]

# measured sample sizes of the reference (hostile_pictures.YUY2_CASES' docstring), 8-bit YUY2: (picture, quality) -> bytes
SIZES_336x252 = {("flat0", 4): 11564, ("flat128", 4): 9176, ("flat255", 4): 11564, ("vstripes", 4): 62488, ("hstripes", 4): 61988, ("checker", 4): 54052, ("impulses", 4): 9340,
                 ("step", 4): 15828, ("flat0", 1): 10484, ("flat128", 1): 9176, ("flat255", 1): 10484, ("noise", 1): 141832, ("vstripes", 1): 38364, ("hstripes", 1): 38176,
                 ("checker", 1): 35528, ("impulses", 1): 9260, ("step", 1): 13780}
SIZES_2048x72 = {"flat0": 13580, "flat128": 13580, "flat255": 13580, "vstripes": 105552, "hstripes": 105552, "checker": 91728, "impulses": 13708, "step": 14692}


def _pin(frame, w, h, quality, fmt, size=None):
    uyvy = int(fmt == "2vuy")
    pixfmt = PIX_2VUY if uyvy else PIX_YUY2
    plan = Plan(w, h, pixkind=PIXKIND[fmt], quality=quality)
    coeffs = oracle_forward_yuv422(plan, frame, 2 * w, uyvy=uyvy)
    predicted = product_write_sample_host(plan, coeffs, 1, input_format=COLOR_FORMAT_UYVY if uyvy else COLOR_FORMAT_YUYV)
    assert H.legal_for_reference(predicted, w, h, 2), "not a legal case: %d bytes predicted" % len(predicted)
    s = ref_encode_frames([frame], 2 * w, w, h, pixfmt, quality=quality)[0]
    if size is not None: assert len(s) == size
    off, m = first_metadata_chunk(s)
    want = product_write_sample_host(plan, coeffs, 1, meta_global=s[off:off + m], input_format=COLOR_FORMAT_UYVY if uyvy else COLOR_FORMAT_YUYV)
    assert len(s) == len(want) and mask_volatile_metadata(s) == mask_volatile_metadata(want)
    deq = oracle_decode_pyramid(s, plan)
    lo, hi = oracle_inverse_yuv422(plan, deq, 0, uyvy=uyvy)[:h], oracle_inverse_yuv422(plan, deq, 1, uyvy=uyvy)[:h]
    def leg():                                            # (the reference decoder answers differently late in a long process: cfhd_testlib.reference_leg)
        out, rp = ref_decode_sample(s, w, h, pixfmt)
        img = out.reshape(h, rp)[:, : 2 * w]
        return bool(((img == lo) | (img == hi)).all())
    assert reference_leg(leg, 3, "hostile 4:2:2 -> 8-bit 4:2:2 (oracle pin)")


@pytest.mark.parametrize("fmt", ["YUY2", "2vuy"])
@pytest.mark.parametrize("name,quality", H.YUY2_CASES)
def test_intra_422_cases(name, quality, fmt):
    _pin(H.yuy2(name, 336, 252, fmt).reshape(-1), 336, 252, quality, fmt, SIZES_336x252[(name, quality)])


@pytest.mark.parametrize("name", H.STRIP_CASES)
def test_strip_cases(name):
    _pin(H.yuy2(name, H.STRIP_W, H.STRIP_H).reshape(-1), H.STRIP_W, H.STRIP_H, QUALITY_FILMSCAN1, "YUY2", SIZES_2048x72.get(name))


@pytest.mark.parametrize("name", H.OVERSIZE)
def test_oversize_cases_are_oversize(name):
    """No reference call: the oracle + host writer predict a sample beyond the reference's whole buffer (w * h * 2 + 64 KB); the sizes are those of hostile_pictures' table."""
    plan = Plan(336, 252)
    s = product_write_sample_host(plan, oracle_forward_yuv422(plan, H.yuy2(name, 336, 252).reshape(-1), 672), 1)
    assert len(s) + 96 == {"noise": 244328, "bw": 283836}[name] and len(s) > 336 * 252 * 2 + 65536          # (+ 96: the encoder's metadata block, which this sample lacks)


# ---- the other transform families (hostile_pictures.FAMILY_CASES): reference encoder == oracle + host writer at the measured size, reference decoder == oracle's inverse

def _pin16(frame, pitch, w, h, bpp, pixfmt, encoded, plan, coeffs, input_format, size, exact_of, what, racy=False, dplan=None):
    predicted = product_write_sample_host(plan, coeffs, 1, input_format=input_format, color_space=0)
    assert H.legal_for_reference(predicted, w, h, bpp), "not a legal case: %d bytes predicted" % len(predicted)
    s = ref_encode_frames([frame], pitch, w, h, pixfmt, encoded=encoded)[0]
    assert len(s) == size
    off, m = first_metadata_chunk(s)
    assert product_write_sample_host(plan, coeffs, 1, meta_global=s[off:off + m], input_format=input_format, color_space=0) == s
    dplan = dplan or plan
    exact, accept = exact_of(dplan, oracle_decode_pyramid(s, dplan))
    def leg():
        r, rp = ref_decode_sample(s, w, h, pixfmt)
        return accept(np.frombuffer(r.tobytes(), np.uint16).reshape(h, rp // 2)[:, : exact.shape[1]])
    assert reference_leg(leg, 3, what, racy=racy) or racy


@pytest.mark.parametrize("name", ["checker", "noise"])
def test_rg48_cases(name):
    w, h = 320, 240
    frame = H.words16(name, h, w, 3).reshape(-1).view(np.uint8).copy()
    plan = Plan(w, h, pixkind=PIXKIND["RG48"], enc=3)
    def exact_of(p, deq):
        e = oracle_inverse_rgb48(p, deq)[:h]
        return e, lambda img: np.array_equal(img, e)
    _pin16(frame, w * 6, w, h, 6, PIX_RG48, ENCODED_RGB444, plan, oracle_forward_planes(plan, rg48_planes(frame, w * 6, w, h)), COLOR_FORMAT_RG48, H.FAMILY_SIZES["RG48 " + name], exact_of, "hostile RGB 4:4:4 -> RG48 (oracle pin)")


def test_b64a_case():
    w, h = 320, 240
    frame = H.b64a_checker_alternating_alpha(w, h).reshape(-1).view(np.uint8).copy()
    plan = Plan(w, h, pixkind=PIXKIND["b64a"], enc=ENC["4444"], quality=QUALITY_FILMSCAN1 | 0x20000000)
    def exact_of(p, deq):
        e = oracle_inverse_rgb48(p, deq, b64a=True)[:h]; raw = oracle_inverse_rgb48(p, deq, b64a=False)[:h]
        def accept(b):                                     # colour exact; an alpha row expanded or, where the reference's workers raced (bayer.c:13871 / :16034), still companded
            colour = all(np.array_equal(b[:, k::4], e[:, k::4]) for k in (1, 2, 3))
            rows = (b[:, 0::4] == e[:, 0::4]).all(axis=1) | (b[:, 0::4] == raw[:, 3::4]).all(axis=1)
            return bool(colour and rows.all())
        return e, accept
    _pin16(frame, w * 8, w, h, 8, PIX_B64A, ENCODED_RGBA4444, plan, oracle_forward_planes(plan, b64a_planes(frame, w * 8, w, h)), COLOR_FORMAT_B64A, H.FAMILY_SIZES["b64a"], exact_of,
           "hostile RGBA 4:4:4:4 -> b64a (oracle pin)", dplan=Plan(w, h, pixkind=PIXKIND["b64a"], enc=ENC["4444"]))


def test_byr4_case():
    w, h = 192, 96
    mosaic = H.words16("checker", h, w, 1)
    plan = Plan(w, h, pixkind=PIXKIND["BYR4"], enc=ENC["bayer"])
    def exact_of(p, deq):
        e = oracle_inverse_byr4(p, deq)[:h, :w]
        return e, lambda img: np.array_equal(img, e)
    _pin16(mosaic.reshape(-1).view(np.uint8).copy(), w * 2, w, h, 2, PIX_BYR4, ENCODED_BAYER, plan, oracle_forward_planes(plan, byr4_planes(mosaic)), COLOR_FORMAT_BYR4, H.FAMILY_SIZES["BYR4"], exact_of,
           "hostile Bayer -> BYR4 (oracle pin)")


def test_interlaced_case():
    w, h = 320, 64
    frame = H.yuy2("hstripes", w, h).reshape(-1)
    plan = Plan(w, h, progressive=0)
    coeffs = oracle_forward_interlaced_yuv422(plan, frame, 2 * w)
    assert H.legal_for_reference(product_write_sample_host(plan, coeffs, 1, progressive=0), w, h, 2)
    s = ref_encode_frames([frame], 2 * w, w, h, PIX_YUY2, flags=1)[0]
    assert len(s) == H.FAMILY_SIZES["interlaced"]
    off, m = first_metadata_chunk(s)
    assert mask_volatile_metadata(product_write_sample_host(plan, coeffs, 1, meta_global=s[off:off + m], progressive=0)) == mask_volatile_metadata(s)
    deq = oracle_decode_pyramid(s, plan)
    lo, hi = oracle_inverse_interlaced_yuv422(plan, deq, 0)[:h], oracle_inverse_interlaced_yuv422(plan, deq, 1)[:h]
    def leg():
        out, rp = ref_decode_sample(s, w, h)
        img = out.reshape(h, rp)[:, : 2 * w]
        return bool(((img == lo) | (img == hi)).all())
    assert reference_leg(leg, 3, "hostile interlaced 4:2:2 (oracle pin)")


@pytest.mark.parametrize("first,second", [("flat0", "flat255"), ("flat255", "flat0")])
def test_group_cases(first, second):
    w, h = 320, 240
    frames = [H.yuy2(first, w, h).reshape(-1), H.yuy2(second, w, h).reshape(-1)]
    gp = GopPlan(w, h)
    coeffs = oracle_forward_gop(gp, frames[0], frames[1], 2 * w)
    assert H.legal_for_reference(product_write_gop_host(gp, 0, coeffs, 1), w, h, 2)
    ss = ref_encode_frames(frames + [frames[0]], 2 * w, w, h, flags=ENCODING_FLAGS_2FRAME_GOP)
    assert [len(x) for x in ss[:2]] == [40, H.FAMILY_SIZES["group"]]
    off, m = first_metadata_chunk(ss[1])
    assert mask_volatile_metadata(product_write_gop_host(gp, 0, coeffs, 1, meta_global=ss[1][off:off + m])) == mask_volatile_metadata(ss[1])
    co = oracle_decode_group(ss[1], gp)
    lo, hi = oracle_inverse_gop(gp, co, 0), oracle_inverse_gop(gp, co, 1)
    def leg():
        got = ref_decode_group_frames(ss, w, h, PIX_YUY2)
        return all(got[0][f] is None or bool(((got[0][f] == lo[f][:h]) | (got[0][f] == hi[f][:h])).all()) for f in range(2))
    assert reference_leg(leg, 2, "hostile two-frame group (oracle pin)")
