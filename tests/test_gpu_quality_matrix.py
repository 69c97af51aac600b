"""Every encoded format at every quality word, both ways, on the hardware (run with `pytest -m gpu` on an MI355X): the bodies of tests/quality_matrix.py, which says what
is checked against what.  Everything outside 8-bit 4:2:2 ran at FILMSCAN1 only before this file; no sample made at another quality was ever decoded on the GPU.  The
packed-math primitives of cfhd_gfx950.h are replaced in the emulated twin (tests/test_quality_matrix_emulated.py), so only this run meets the real ones at these quantizers.

Feedback qualities (FILMSCAN2 / FILMSCAN3) reach the strip kernels here through the C ABI's handle (test_strip_kernels_at_the_feedback_qualities_through_the_handle):
the handle honours CFHD_AMD_FORWARD as the batches do, cfhd_amd_encoder_kernel_name is the witness."""
import pytest
from cfhd_testlib import *
import quality_matrix as Q
from test_gpu_parity import _reference_must_be_present      # noqa: F401 (the fixture applies here too)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route,w,h,quality", Q.ENCODE_CASES, ids=Q.case_id)
def test_encode_equals_reference(route, w, h, quality):
    Q.check_encode(route, w, h, quality)


@pytest.mark.parametrize("route,quality", Q.DECODE_CASES, ids=Q.case_id)
def test_decode_of_reference_samples(route, quality):
    Q.check_decode(route, quality)


@pytest.mark.parametrize("route,quality", Q.STRIP_CASES, ids=Q.case_id)
def test_strip_kernels(route, quality):
    Q.check_strip(route, quality)


@pytest.mark.parametrize("route,quality", Q.STRIP_HANDLE_CASES, ids=Q.case_id)
def test_strip_kernels_at_the_feedback_qualities_through_the_handle(route, quality):
    Q.check_strip_handle(route, quality)


@pytest.mark.parametrize("w,h,quality", Q.LIMITER_CASES)
def test_limiter_size_gate(w, h, quality):
    Q.check_limiter_geometry(w, h, quality)


def test_quality_switches_on_one_handle():
    Q.check_quality_switches_on_one_handle()


def test_quality_switches_on_the_pool():
    Q.check_quality_switches_on_the_pool()


@pytest.mark.parametrize("route", Q.REWRITE_ROUTES)
@pytest.mark.parametrize("quality", Q.UNCOMPRESSED_WORDS, ids=hex)
def test_uncompressed_bits_on_inputs_that_cannot_be_stored_raw(route, quality):
    Q.check_uncompressed_bits_on_other_inputs(route, quality)


@pytest.mark.parametrize("fmt", Q.RAW_STORABLE)
def test_uncompressed_mode_is_refused(fmt):
    Q.check_uncompressed_mode_is_refused(fmt)


@pytest.mark.parametrize("fmt,out", [("v210", "v210"), ("r210", "RG48"), ("BYR4", "BYR4")])
def test_uncompressed_samples_are_refused(fmt, out):
    Q.check_uncompressed_samples_are_refused(fmt, out)


def test_fixed_quality_is_refused():
    Q.check_fixed_quality_is_refused()


@pytest.mark.parametrize("route,refused,taken", Q.NARROW)
def test_narrow_frames_are_refused(route, refused, taken):
    Q.check_narrow_frames_are_refused(route, refused, taken)


def test_limiter_size_bound():
    Q.check_limiter_size_bound()
