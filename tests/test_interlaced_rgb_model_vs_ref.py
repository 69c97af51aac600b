"""Pins tests/interlaced_rgb_model.py -- the reference's full-resolution RG48 / b64a / BGRA / BGRa decode of interlaced 4:2:2 samples (decoder.c:22027
TransformInverseFrameToRow16u + bayer.c:13186 ConvertRow16uToOutput) -- on the reference decoder itself, on samples its encoder writes with
CFHD_ENCODING_FLAGS_YUV_INTERLACED.  CPU only: the GPU route (k_inv_frame_yuv422_rows16 + k_yu64_to_rgb16) is held to this model by test_gpu_interlaced_rgb.py."""
import numpy as np
import pytest
from cfhd_testlib import *
from interlaced_rgb_model import model_decode, interlaced_row16u

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not have_ref(), reason="reference .so not built")]

INTERLACED = 1          # CFHD_ENCODING_FLAGS_YUV_INTERLACED
MATRIX_601 = 4          # (the flag that makes the reference encoder tag the sample 601, as in test_oracle_vs_ref)


def interlaced_sample(w, h, flags):
    """An interlaced reference sample whose picture runs into both clips of the colour conversion, its fields apart."""
    f, p = synth_yuy2(w, h, w + h)
    v = f.reshape(h, p)
    v[: h // 6, 0::2] = np.linspace(0, 255, w).astype(np.uint8)[None, :]
    v[h // 6: h // 3, 1::4] = 255; v[h // 6: h // 3, 3::4] = 0
    v[h // 3: h // 2, 1::4] = 0; v[h // 3: h // 2, 3::4] = 255
    v[1::2] = np.roll(v[1::2], 8, axis=1)
    return ref_encode_frames([f], p, w, h, flags=flags | INTERLACED)[0]


def ref_view(sample, w, h, name):
    dec, dpitch = ref_decode_sample(sample, w, h, fourcc(name))
    if name in ("BGRA", "BGRa"):
        return np.frombuffer(dec.tobytes(), np.uint8).reshape(-1, dpitch)[:h, : w * 4]
    nw = {"YU64": 2, "RG48": 3, "b64a": 4}[name]
    return np.frombuffer(dec.tobytes(), np.uint16).reshape(-1, dpitch // 2)[:h, : w * nw]


def pin(sample, w, h, name, want):
    """The reference's output equals `want`.  Through reference_leg: the reference's 16-bit routes are known to answer differently late in a long process
    (uninitialised rows, cfhd_testlib.ref_decode_sample_fresh_process); a few runs here, then a fresh process, and a disagreement there fails the test."""
    def leg():
        got = ref_view(sample, w, h, name)
        return (got.shape == want.shape and np.array_equal(got, want)) or "%d values differ from the model" % (got != want).sum()
    assert reference_leg(leg, 3, "interlaced 4:2:2 -> %s (model pin)" % name)


GEOMETRIES = [(320, 240, 0), (336, 252, MATRIX_601), (720, 486, MATRIX_601), (1280, 720, 0), (1920, 1080, 0)]


@pytest.mark.parametrize("w,h,flags", GEOMETRIES)
@pytest.mark.parametrize("name", ["YU64", "RG48", "b64a", "BGRA"])
def test_reference_interlaced_rows16_and_rgb_equal_model(w, h, flags, name):
    """Word for word (YU64: the 16-bit rows themselves; RG48 / b64a) and byte for byte (BGRA, bottom row first): 709 and 601, a band width with a tail that is not
    a multiple of 8 columns (336: luma band 168, chroma band 84), a display height below the coded height (486 of 488), 1080i."""
    sample = interlaced_sample(w, h, flags)
    pin(sample, w, h, name, model_decode(sample, w, h, name, 1 if flags & MATRIX_601 else 2))


@pytest.mark.parametrize("name", ["YU64", "RG48", "b64a", "BGRA"])
def test_reference_interlaced_qbist_1080i_equals_model(name):
    frames, pitch = qbist_frames(10, 1)
    sample = ref_encode_frames(frames, pitch, 1920, 1080, flags=INTERLACED)[0]
    pin(sample, 1920, 1080, name, model_decode(sample, 1920, 1080, name, 2))


@pytest.mark.parametrize("name", ["YU64", "RG48", "b64a", "BGRA"])
def test_reference_interlaced_field_flicker_with_peak_table_equals_model(name):
    """The difference band of a field-flicker frame carries a peak table (values beyond +-250 quantization steps)."""
    w, h = 320, 64
    frames = [synth_yuy2(w, h, 3)[0], field_flicker_frame(w, h)[0]]
    samples = ref_encode_frames(frames, w * 2, w, h, PIX_YUY2, flags=INTERLACED)
    assert len(samples[1]) != len(samples[0])
    for smp in samples:
        pin(smp, w, h, name, model_decode(smp, w, h, name, 2))


def test_bgra_model_is_rg48_words_shifted_and_flipped():
    """BGRA is the RG48 picture at white point 16 >> 8 (bayer.c:825, no dither), bottom row first; BGRa the same bytes top row first.  The reference's own BGRa of an
    interlaced sample is not this picture -- its interlaced switch (decoder.c:26488) has no case for DECODED_FORMAT_RGB32_INVERTED -- so BGRa is held to the BGRA
    bytes the reference gives, read top row first."""
    w, h = 320, 240
    sample = interlaced_sample(w, h, 0)
    rg48 = model_decode(sample, w, h, "RG48", 2).reshape(h, w, 3)
    bgra = model_decode(sample, w, h, "BGRA", 2).reshape(h, w, 4)
    bgra_top = model_decode(sample, w, h, "BGRa", 2).reshape(h, w, 4)
    assert np.array_equal(bgra[::-1], bgra_top)
    assert np.array_equal(bgra_top[:, :, 2], rg48[:, :, 0] >> 8) and np.array_equal(bgra_top[:, :, 0], rg48[:, :, 2] >> 8)
    assert (bgra_top[:, :, 3] == 255).all()
    pin(sample, w, h, "BGRA", bgra_top.reshape(h, -1)[::-1])


def test_row16u_tail_equals_vector_body_in_range():
    """temporal.c:7087: the scalar tail ((x) / 2, clamp [0, 1023], << 6) and the vector body (clamp [0, 2047], >> 1, << 6) give the same words for every sum a
    decoder meets; they part only far below zero (the adds / subs_epu16 pair wraps there)."""
    lo = np.arange(-4096, 4096, 3, dtype=np.int32)[None, :].repeat(2, 0)
    hi = np.zeros_like(lo); hi[1] = 7
    width = lo.shape[1] - lo.shape[1] % 8
    vec_even, vec_odd = interlaced_row16u(lo[:, :width], hi[:, :width])
    tail_even, tail_odd = interlaced_row16u(lo[:, :7], hi[:, :7])          # (seven columns: all of them the scalar tail)
    assert np.array_equal(vec_even[:, :7], tail_even) and np.array_equal(vec_odd[:, :7], tail_odd)
    assert vec_even.max() == 1023 << 6 and vec_even.min() == 0
