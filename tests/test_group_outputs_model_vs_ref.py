"""Pins tests/group_outputs_model.py -- a two-frame group decoded to the outputs of a 4:2:2 sample other than full-resolution 8-bit 4:2:2 -- on the reference's own group
decoder, on streams its encoder writes with CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP (and _YUV_INTERLACED).  CPU only: the GPU route is held to this model by
test_gpu_group_outputs.py.  The reference is driven as cfhd_testlib.ref_decode_group_frames documents (test_gpu_group_outputs.ref_group_outputs); its pictures are
cropped by the output's own pitch.  Exact for every output but full-resolution RG24, whose 15-bit rand() dither is held to the interval of the intra RG24 gate."""
import numpy as np
import pytest
from cfhd_testlib import *
import group_outputs_model as M
from test_gpu_group_outputs import group_stream, ref_group_outputs, rg24_in_interval, source_rgb24, MATRIX_601

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not have_ref(), reason="reference .so not built")]

# (w, h, fmt, interlaced, flicker, flags)
GEOMETRIES = [(320, 240, "YUY2", 0, 0, 0), (336, 252, "YUY2", 0, 0, 0), (336, 252, "YUY2", 0, 0, MATRIX_601), (720, 486, "2vuy", 0, 0, MATRIX_601),
              (1920, 1080, "YUY2", 0, 0, 0), (384, 96, "YUY2", 0, 0, MATRIX_601),
              (336, 252, "YUY2", 1, 0, 0), (336, 252, "YUY2", 1, 1, MATRIX_601), (720, 486, "2vuy", 1, 1, 0)]


def pin(samples, gp, name, half, color_space):
    got, aw, ah, pitch = ref_group_outputs(samples, name, half)
    rows = 2 * ah if half else ah
    checked = 0
    for g, pair in enumerate(got):
        want = M.model_decode_group(samples[2 * g + 1], gp, name, rows, color_space, half)
        for f, raw in enumerate(pair):
            if raw is None: continue
            img = M.view_output(raw, pitch, aw, ah, name)
            if name == "RG24" and not half:
                verdict = rg24_in_interval(img, want[f], source_rgb24(gp, 2 * g + f, rows, color_space if f == 0 else 2), (0.4, 0.6))
                assert verdict is True, "group %d frame %d: %s" % (g, f, verdict)
            else:
                assert img.shape == want[f].shape and np.array_equal(img, want[f]), "%s%s group %d frame %d: %d values differ from the model" % (
                    name, " (half)" if half else "", g, f, (img != want[f]).sum())
            checked += 1
    assert checked >= 3


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("w,h,fmt,interlaced,flicker,flags", GEOMETRIES)
def test_reference_group_outputs_equal_model(w, h, fmt, interlaced, flicker, flags, half):
    """Every output the product serves for this stream (tests/group_outputs_model.py served, FULL_* / HALF* lists): YU64, v210, BGRA, BGRa (progressive), RG48, b64a and
    every half-resolution output word for word / byte for byte; RG24 at full resolution inside its dither interval.  709 and 601 (the 601 tag holds for frame 0 only:
    the P-frame sample that hands out frame 1 carries no colour space tag)."""
    samples, gp = group_stream(w, h, fmt, interlaced, flicker, flags)
    if half: names = M.HALF_INTERLACED if interlaced else M.HALF
    else: names = [n for n in M.FULL_INTERLACED if n != "BGRa"] if interlaced else M.FULL_PROGRESSIVE
    for name in names:
        if M.served(name, w, bool(half)): pin(samples, gp, name, bool(half), 1 if flags & MATRIX_601 else 2)


def test_interlaced_group_bgra_top_row_first_is_bgra_flipped():
    """Interlaced groups, BGRa: the BGRA bytes read top row first, as for intra samples -- the reference's own BGRa of an interlaced picture is not the picture (its
    interlaced switch has no case for inverted RGB32: test_interlaced_rgb_model_vs_ref.test_bgra_model_is_rg48_words_shifted_and_flipped).  (At even lowpass widths: at odd
    ones the two formats take different lowpass biases, group_lowpass_bias.)"""
    samples, gp = group_stream(320, 240, "YUY2", 1, 0, 0)
    bgra = M.model_decode_group(samples[1], gp, "BGRA", 240)
    bgra_top = M.model_decode_group(samples[1], gp, "BGRa", 240)
    for f in range(2): assert np.array_equal(bgra[f][::-1], bgra_top[f])
    got, aw, ah, pitch = ref_group_outputs(samples, "BGRA", False)
    assert np.array_equal(M.view_output(got[0][0], pitch, aw, ah, "BGRA"), bgra[0])


def test_group_lowpass_bias_differs_from_twice_the_intra_bias_where_the_reference_says():
    """The reference's table of group lowpass biases (decoder.c:12265-12278, :12486-12510) against twice the intra bias: equal for the 8-bit 4:2:2 outputs and RG48 / b64a;
    14 instead of 8 for YU64 / v210 at even widths; at odd widths the RGB24 / RGB32 correction is added once.  The decode of YU64 with twice the intra bias misses the
    reference's picture."""
    for width in (40, 42, 90):
        for name in ("YUY2", "RG48", "b64a", "BGRa"):
            for c in range(3): assert M.group_lowpass_bias(width, name, c) == 2 * oracle_lowpass_bias(10, width, PIXKIND[name], c)
    assert M.group_lowpass_bias(40, "YU64", 0) == 14 != 2 * oracle_lowpass_bias(10, 40, PIXKIND["YU64"], 0)
    assert [M.group_lowpass_bias(21, "BGRA", c) for c in range(3)] == [2, 6, 6]
    samples, gp = group_stream(320, 240, "YUY2", 0, 0, 0)
    got, aw, ah, pitch = ref_group_outputs(samples, "YU64", False)
    img = M.view_output(got[0][0], pitch, aw, ah, "YU64")
    assert np.array_equal(img, M.model_decode_group(samples[1], gp, "YU64", ah)[0])
    twice = oracle_decode_group(samples[1], gp, lowpass_offset=0)
    for c in range(3):
        d = gp.w[(c, 5)]
        gp.view(twice, c, 5, 0)[:, : d["width"]] += 2 * oracle_lowpass_bias(10, d["width"], PIXKIND["YU64"], c)
    work = M.level1_wavelets(gp, twice)
    assert not np.array_equal(img, M.finish_frame(M.FramePlanOfGroup(gp, 0, ah), work, "YU64", 2, False, False))
