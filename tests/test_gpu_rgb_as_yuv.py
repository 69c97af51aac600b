"""RGB 4:4:4 and RGBA 4:4:4:4 samples delivered as the reference's YU64 picture on the MI355X: cfhd_amd_decode_batch_set_device_pictures with the RGB_AS_* layouts
(k_dec_deliver_rgb_as_yuv -- every product and sum a single of its own, v_mul_f32 and v_add_f32 and no fused multiply-add, the conversion v_cvt_i32_f32, the f16
rounding the hardware's convert).  tests/rgb_as_yuv.py has the bodies; tests/test_rgb_as_yuv_emulated.py runs them on the CPU."""
import importlib.util, os, subprocess, sys
if __name__ == "__main__": import torch      # (the child of the last test: torch before anything of the library's, as bench.py has it)
import pytest
from cfhd_testlib import *
import rgb_as_yuv as RY

pytestmark = pytest.mark.gpu
LAYOUT_IDS = [RY.LAYOUT_NAMES[l] for l in RY.LAYOUTS]


@pytest.mark.parametrize("name", RY.DELIVERY_IDS)
def test_delivery_equals_the_model_on_the_pass_own_pictures_and_the_reference(name):
    RY.check_delivery(name)


@pytest.mark.parametrize("layout", [RY.RGB_AS_YU64, RY.RGB_AS_YUV422_F16], ids=["yu64", "f16"])
def test_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(layout):
    RY.check_short_pass_and_switching(layout)


@pytest.mark.parametrize("layout", RY.LAYOUTS, ids=LAYOUT_IDS)
def test_a_mixed_pass_converts_every_picture_with_the_matrix_of_its_own_sample(layout):
    RY.check_mixed_pass(layout)


@pytest.mark.parametrize("layout", RY.LAYOUTS, ids=LAYOUT_IDS)
def test_a_failed_sample_is_zeros_and_its_neighbours_are_intact(layout):
    RY.check_failed_samples(layout)


@pytest.mark.parametrize("layout", [RY.RGB_AS_YU64, RY.RGB_AS_YUV422_U16], ids=["yu64", "u16"])
def test_both_submit_paths_deliver_and_host_delivery_is_unchanged_beside_it(layout):
    RY.check_submit_paths(layout)


def test_gates():
    RY.check_gates()


def test_the_kernel_time_and_name_follow_the_layout():
    RY.check_kernel_times()


def test_one_row_of_a_torch_tensor_views_as_y_and_cbcr():
    """In a child process that imports torch before the library is loaded, as bench.py does: torch brings a HIP runtime of its own, and the process that runs this
    suite has long loaded the library's."""
    if importlib.util.find_spec("torch") is None: pytest.skip("no torch")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "torch"], capture_output=True, text=True, timeout=300)
    if "TORCH SEES NO DEVICE" in run.stdout: pytest.skip("torch sees no device")
    assert run.returncode == 0 and "TORCH OK" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def _torch_child():
    import torch
    if not torch.cuda.is_available(): print("TORCH SEES NO DEVICE"); return
    RY.check_torch(torch)
    print("TORCH OK")


if __name__ == "__main__":
    _torch_child()
