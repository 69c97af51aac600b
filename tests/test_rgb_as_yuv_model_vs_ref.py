"""tests/rgb_as_yuv_model.py against the reference decoder, on the CPU: the reference's YU64 decode of an RGB 4:4:4 or RGBA 4:4:4:4 sample equals the model applied to
the reference's own RG48 decode of the same sample, word for word -- five geometries, samples encoded without and with CFHD_ENCODING_FLAGS bit 8 (the encoder then
writes the colour-space tag with bit 2 set) and with that tag patched to 1, 5 and 6.  The pictures carry patches of white, black, the primaries, yellow and cyan:
under the video-systems matrix both 65535 and 0 are reached, and the test says so.  Every decode has a reference handle of its own, in a child process per case
(rgb_as_yuv.ref_consistent_pairs).  The reference's threaded decoder now and then returns a damaged picture -- stretches, a whole component, the words beside a
saturated edge --, as tests/test_oracle_vs_ref.py knows: each picture gets rgb_as_yuv.REF_ATTEMPTS decodes to show the pair that satisfies the statement, which no
damaged picture does by accident; the attempts each case needed are printed.  Skipped where oracle/_ref is not built."""
import numpy as np
import pytest
from cfhd_testlib import *
import rgb_as_yuv as RY
import rgb_as_yuv_model as M

pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref is not built")
GEOMETRIES = [(72, 40), (192, 96), (200, 64), (504, 242), (1920, 1080)]
LEGS = ["444", "4444"]                                          # RG48 -> RGB 4:4:4, b64a -> RGBA 4:4:4:4
PATCHED_TAGS = (1, 5, 6)


@pytest.mark.parametrize("w,h", GEOMETRIES, ids=["%dx%d" % g for g in GEOMETRIES])
@pytest.mark.parametrize("leg", LEGS)
def test_the_reference_yu64_picture_is_the_model_of_its_rg48_picture(leg, w, h):
    plain = RY.samples_of(leg, w, h, 1, 0, "ref")[0]
    flagged = RY.samples_of(leg, w, h, 1, RY.FLAG_VIDEO_SYSTEMS, "ref")[0]
    assert M.color_space_tag(plain) is None, "the reference tags an RGB sample it was not asked to tag"
    tag = M.color_space_tag(flagged)
    assert tag is not None and tag & 4, "flag bit 8 did not tag the sample as video systems (tag %r)" % tag
    if leg == "444": assert len(flagged) == len(plain) + 4       # (the tag-value pair; the RGBA encoder's bands change with the flag as well)
    samples = [plain, flagged] + [M.with_tag(flagged, v) for v in PATCHED_TAGS]
    tags = [0, tag] + list(PATCHED_TAGS)
    assert [RY.tag_of(s) for s in samples] == tags
    pairs = RY.ref_consistent_pairs(samples, w, h, tags)
    lo, hi = 65535, 0
    for t, (rg48, yu64, counts) in zip(tags, pairs):
        print("%s %d x %d, tag %d: words of the model that differ from the reference's YU64 picture, per attempt: %s" % (leg, w, h, t, counts))
        assert counts[-1] == 0, "%s %d x %d, tag %d: no pair of the reference's pictures satisfies the model in %d attempts (words that differ: %s)" % (leg, w, h, t, len(counts), counts)
        assert rg48.shape == (h, 6 * w) and yu64.shape == (h, 4 * w)
        got = M.yu64_of_rg48(rg48, w, h, t)
        assert np.array_equal(got.view(np.uint16), np.ascontiguousarray(yu64).view(np.uint16))
        if t & 4:
            words = np.ascontiguousarray(yu64).view(np.uint16)
            lo, hi = min(lo, int(words.min())), max(hi, int(words.max()))
            assert not np.array_equal(M.yu64_of_rg48(rg48, w, h, 0), got), "the two matrices give the same picture: the test shows nothing"
    assert (lo, hi) == (0, 65535), "under the video-systems matrix the pictures reach %d .. %d, not both ends" % (lo, hi)
