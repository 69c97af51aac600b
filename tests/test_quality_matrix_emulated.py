"""tests/test_gpu_quality_matrix.py on the CPU against the emulated product library (cfhd_testlib.emulated_product): the same bodies (tests/quality_matrix.py) on a
subset -- every route at LOW and FILMSCAN3, every word on one route per encoded format, the decode matrix likewise, the strip kernels on the narrowest geometries, and
all of the rewritten and refused quality words.  The emulator replaces the packed-math primitives of cfhd_gfx950.h (tests/hipemu/cfhd_gfx950.h): what this file pins is
the host derivation, the job tables and the kernels' C++; the gfx950 build of the same kernels is the GPU file's."""
import pytest
from cfhd_testlib import *
import quality_matrix as Q

pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")


@pytest.mark.parametrize("route,w,h,quality", Q.EMULATED_ENCODE_CASES, ids=Q.case_id)
def test_emulated_encode_equals_reference(route, w, h, quality):
    with emulated_product(): Q.check_encode(route, w, h, quality)


@pytest.mark.parametrize("route,quality", Q.EMULATED_DECODE_CASES, ids=Q.case_id)
def test_emulated_decode_of_reference_samples(route, quality):
    with emulated_product(): Q.check_decode(route, quality)


@pytest.mark.parametrize("route,quality", Q.EMULATED_STRIP_CASES, ids=Q.case_id)
def test_emulated_strip_kernels(route, quality):
    with emulated_product(): Q.check_strip(route, quality)


@pytest.mark.parametrize("route,quality", Q.EMULATED_STRIP_HANDLE_CASES, ids=Q.case_id)
def test_emulated_strip_kernels_at_the_feedback_qualities_through_the_handle(route, quality):
    with emulated_product(): Q.check_strip_handle(route, quality)


def test_emulated_quality_switches_on_one_handle():
    with emulated_product(): Q.check_quality_switches_on_one_handle()


def test_emulated_quality_switches_on_the_pool():
    with emulated_product(): Q.check_quality_switches_on_the_pool()


@pytest.mark.parametrize("route", Q.REWRITE_ROUTES)
@pytest.mark.parametrize("quality", Q.UNCOMPRESSED_WORDS, ids=hex)
def test_emulated_uncompressed_bits_on_inputs_that_cannot_be_stored_raw(route, quality):
    with emulated_product(): Q.check_uncompressed_bits_on_other_inputs(route, quality)


@pytest.mark.parametrize("fmt", Q.RAW_STORABLE)
def test_emulated_uncompressed_mode_is_refused(fmt):
    with emulated_product(): Q.check_uncompressed_mode_is_refused(fmt)


@pytest.mark.parametrize("fmt,out", [("v210", "v210"), ("r210", "RG48"), ("BYR4", "BYR4")])
def test_emulated_uncompressed_samples_are_refused(fmt, out):
    with emulated_product(): Q.check_uncompressed_samples_are_refused(fmt, out)


def test_emulated_fixed_quality_is_refused():
    with emulated_product(): Q.check_fixed_quality_is_refused()


@pytest.mark.parametrize("route,refused,taken", Q.NARROW)
def test_emulated_narrow_frames_are_refused(route, refused, taken):
    with emulated_product(): Q.check_narrow_frames_are_refused(route, refused, taken)


def test_emulated_limiter_size_bound():
    with emulated_product(): Q.check_limiter_size_bound()
