"""tests/test_gpu_interlaced_rgb.py on the CPU against the emulated product library (cfhd_testlib.emulated_product, as tests/test_product_emulated.py does for the
rest of the GPU suite): the job tables of the interlaced RG48 / b64a / BGRA / BGRa route -- the scratch frame, the 16-bit-row kernel, the conversion's 8-bit
mode -- checked against the model before any hardware run.  Sizes up to 720 x 486.  Test infrastructure only."""
import pytest
from cfhd_testlib import *
import test_gpu_interlaced_rgb as G

pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")


@pytest.mark.parametrize("w,h,name,flags", [(320, 240, "RG48", 0), (320, 240, "BGRa", 0), (336, 252, "b64a", G.MATRIX_601), (336, 252, "BGRA", 0),
                                            (720, 486, "BGRA", G.MATRIX_601), (720, 486, "RG48", G.MATRIX_601)])
def test_emulated_interlaced_rgb_decode_equals_model(w, h, name, flags):
    with emulated_product():
        G.test_interlaced_rgb_decode_equals_model(w, h, name, flags)


def test_emulated_interlaced_rgb_decode_of_peak_table_flicker_frames():
    with emulated_product():
        G.test_interlaced_rgb_decode_of_peak_table_flicker_frames()


@pytest.mark.parametrize("name", ["BGRA", "RG48"])
def test_emulated_one_handle_alternates_interlaced_and_progressive(name):
    with emulated_product():
        G.test_one_handle_alternates_interlaced_and_progressive(name)


def test_emulated_concurrent_interlaced_rgb_decoders():
    with emulated_product():
        G.test_concurrent_interlaced_rgb_decoders_gather_and_stay_exact()


@pytest.mark.parametrize("name", ["YU64", "v210", "RG24", "r210"])
def test_emulated_remaining_interlaced_full_resolution_gates(name):
    with emulated_product():
        G.test_remaining_interlaced_full_resolution_gates(name)
