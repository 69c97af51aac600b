"""tests/test_gpu_group_outputs.py on the CPU against the emulated product library (cfhd_testlib.emulated_product, as tests/test_interlaced_rgb_emulated.py does): the
GopBatch job tables of every group output -- the YU64 scratch pair, the intra last-level and half-resolution kernels on the group pyramid, the conversions over both
frames, the lowpass bias of the requested output on both entropy stages -- checked against the model before any hardware run.  Sizes up to 720 x 486."""
import pytest
from cfhd_testlib import *
import test_gpu_group_outputs as G

pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("w,h,fmt,interlaced,flicker,flags", [c for c in G.CASES if c[0] <= 720])
def test_emulated_group_outputs_equal_model(w, h, fmt, interlaced, flicker, flags, half):
    with emulated_product():
        G.test_group_outputs_equal_model(w, h, fmt, interlaced, flicker, flags, half)


@pytest.mark.parametrize("w,h,fmt,interlaced,flicker,flags", [(336, 252, "YUY2", 0, 0, G.MATRIX_601), (336, 252, "YUY2", 1, 1, 0)])
def test_emulated_group_outputs_with_host_entropy(w, h, fmt, interlaced, flicker, flags):
    with emulated_product():
        G.test_group_outputs_with_host_entropy(w, h, fmt, interlaced, flicker, flags)


def test_emulated_interlaced_group_rows16_one_column_kernel():
    with emulated_product():
        G.test_interlaced_group_rows16_one_column_kernel()


def test_emulated_one_handle_reprepared_across_outputs_and_resolutions():
    with emulated_product():
        G.test_one_handle_reprepared_across_outputs_and_resolutions()


def test_emulated_group_prepare_gates():
    with emulated_product():
        G.test_group_prepare_gates()


@pytest.mark.parametrize("name,half,w", G.REFUSALS)
def test_emulated_interlaced_group_refusals_then_next_sample(name, half, w):
    with emulated_product():
        G.test_interlaced_group_refusals_then_next_sample(name, half, w)
