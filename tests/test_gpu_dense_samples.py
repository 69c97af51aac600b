"""Dense samples on the real kernels (run with `pytest -m gpu` on an MI355X): the batched encoder writes every sample at its 64-byte aligned offset of one buffer
(k_ent_sizes, k_ent_pack_offsets, k_ent_layout, k_ent_emit) and the decoder parses them there (k_dec_parse with offsets).  Batches of five frames of very different sizes
-- black, grey, Qbist, uniform noise, Qbist again -- through cfhd_amd_batch_*, at a width that takes the block-list path (256) and one that counts level 1 densely (176).

  samples: masked, the reference encoder's -- except the noise frame: its sample is larger than w * h * 2 bytes, where the reference overruns its own buffer
           (hostile_pictures.legal_for_reference); that frame is held to the oracle's transform + the host writer, byte for byte, as tests/test_gpu_hostile.py does
  pictures: every byte inside the oracle's dither interval
  places: every sample starts 64-byte aligned behind the one in front, none overlaps
  a second pass on the same batch object with the pictures permuted: the same checks (offsets of the first pass must not survive)

GPU-side statistics do not tell whether a segment took k_ent_emit's wide path; tests/test_dense_samples_emulated.py asserts it for the same noise frame under emulation."""
import ctypes
import numpy as np
import pytest
from cfhd_testlib import *
import hostile_pictures as H
from test_gpu_parity import _batch_api, _reference_must_be_present      # noqa: F401 (the fixture applies here too)
from test_dense_samples_emulated import five_frames, peak_levels

pytestmark = pytest.mark.gpu


def _samples_and_pictures(L, b, n, w, h):
    got = []
    for i in range(n):
        p = ctypes.c_void_p(); sz = ctypes.c_size_t()
        assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
        out = np.zeros(h * w * 2, np.uint8)
        assert L.cfhd_amd_batch_download_output(b, i, out.ctypes.data_as(ctypes.c_void_p), 2 * w) == 0
        got.append((p.value, sz.value, ctypes.string_at(p, sz.value), out.reshape(h, 2 * w)))
    return got


def _check_places(got):
    base = got[0][0]
    at = 0
    for i, (addr, size, _, _) in enumerate(got):
        assert size > 0
        assert addr - base == at and at % 64 == 0, "sample %d at offset %d, expected %d" % (i, addr - base, at)
        at += (size + 63) & ~63


def _check_pass(L, b, frames, order, w, h, flags, first_number):
    n = len(order)
    for i, k in enumerate(order):
        assert L.cfhd_amd_batch_upload(b, i, frames[k].ctypes.data_as(ctypes.c_void_p), 2 * w) == 0
    assert L.cfhd_amd_batch_roundtrip(b) > 0, amd_last_error()
    got = _samples_and_pictures(L, b, n, w, h)
    _check_places(got)
    plan = Plan(w, h, progressive=0 if flags else 1)
    forward = oracle_forward_interlaced_yuv422 if flags else oracle_forward_yuv422
    inverse = oracle_inverse_interlaced_yuv422 if flags else oracle_inverse_yuv422
    wants = []
    for i, k in enumerate(order):
        sample = got[i][2]
        off, m = first_metadata_chunk(sample)
        wants.append(product_write_sample_host(plan, forward(plan, frames[k], 2 * w), first_number + i, meta_global=sample[off:off + m], progressive=0 if flags else 1))
    # The reference numbers its frames by its calls: one encoder, black frames for the passes in front and in place of a picture that is not legal for it.
    legal = [H.legal_for_reference(x, w, h, 2) for x in wants]
    refs = ref_encode_frames([frames[0]] * (first_number - 1) + [frames[k] if legal[i] else frames[0] for i, k in enumerate(order)], 2 * w, w, h, PIX_YUY2, flags=flags)[first_number - 1:]
    for i, k in enumerate(order):
        _, size, sample, img = got[i]
        if legal[i]:
            assert size == len(refs[i]), "frame %d: %d bytes vs reference %d" % (i, size, len(refs[i]))
            assert mask_volatile_metadata(sample) == mask_volatile_metadata(refs[i]), "frame %d differs from the reference" % i
        assert sample == wants[i], "frame %d differs from the oracle + host writer" % i
        deq = oracle_decode_pyramid(sample, plan)
        lo, hi = inverse(plan, deq, 0)[:h], inverse(plan, deq, 1)[:h]
        ok = (img == lo) | (img == hi)
        assert ok.all(), "frame %d: %d bytes outside the dither interval" % (i, (~ok).sum())
    return got


@pytest.mark.parametrize("w,h", [(256, 144), (176, 96)])
def test_dense_samples_of_a_batch_of_very_different_frames(w, h):
    L = _batch_api()
    frames, pitch = five_frames(w, h)
    assert pitch == 2 * w
    b = L.cfhd_amd_batch_create(w, h, PIX_YUY2, QUALITY_FILMSCAN1, 5, 4)
    assert b, amd_last_error()
    try:
        first = _check_pass(L, b, frames, [0, 1, 2, 3, 4], w, h, 0, 1)
        sizes = [g[1] for g in first]
        assert sizes[3] > 4 * sizes[0] and sizes[3] > w * h * 2      # the noise frame: several times the black one, beyond what the reference's buffer takes
        second = _check_pass(L, b, frames, [3, 0, 4, 1, 2], w, h, 0, 6)      # (the second pass of a batch numbers its frames behind the first's)
        assert [g[1] for g in second] == [sizes[k] for k in (3, 0, 4, 1, 2)]
    finally:
        L.cfhd_amd_batch_destroy(b)


def test_dense_samples_of_an_interlaced_batch_with_peak_tables():
    """Interlaced: the field-flicker picture's difference-coded bands carry peak tables (k_ent_peaks writes them through peak_out, inside the dense buffer), the others none."""
    w, h = 176, 96
    L = _batch_api()
    frames, _ = five_frames(w, h)
    frames[3] = field_flicker_frame(w, h)[0]
    b = L.cfhd_amd_batch_create_ex(w, h, PIX_YUY2, ENCODED_YUV422, 1, QUALITY_FILMSCAN1, 5, 4, 0)
    assert b, amd_last_error()
    try:
        got = _check_pass(L, b, frames, [0, 1, 2, 3, 4], w, h, 1, 1)
        assert any(peak_levels(got[3][2])) and not any(peak_levels(got[0][2]))
    finally:
        L.cfhd_amd_batch_destroy(b)
