"""Thumbnail batches of the decode queue on the MI355X: cfhd_amd_decode_batch_create_thumbnails (k_dec_ingest, k_dec_parse, k_dec_thumbnail -- the 1/8 x 1/8 DPX0
picture of every sample from its raw lowpass words: byte swaps by v_perm_b32, 32-bit integer arithmetic, 16-byte stores) and its delivery, packed (k_dec_deliver) or
as R, G, B planes of the 10-bit values (k_dec_deliver_rgb10; the f16 rounding the hardware's convert).  Every picture is held byte for byte to CFHD_GetThumbnail.
tests/thumbnail_queue.py has the bodies; tests/test_thumbnail_queue_emulated.py runs them on the CPU."""
import importlib.util, os, subprocess, sys
if __name__ == "__main__": import torch      # (the child of the last test: torch before anything of the library's, as bench.py has it)
import pytest
from cfhd_testlib import *
import thumbnail_queue as TQ

pytestmark = pytest.mark.gpu
LAYOUT_IDS = [TQ.LAYOUT_NAMES[l] for l in TQ.LAYOUTS]


@pytest.mark.parametrize("layout", TQ.LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("geometry", TQ.GEOMETRIES, ids=TQ.GEOMETRY_IDS)
def test_every_picture_equals_cfhd_getthumbnail_on_every_way_out(geometry, layout):
    TQ.check_exact(*geometry, layout)


@pytest.mark.parametrize("layout", TQ.LAYOUTS, ids=LAYOUT_IDS)
def test_a_picture_of_several_steps_a_workgroup_and_rows_longer_than_a_wave_step(layout):
    """4224 x 96: 528 x 12 thumbnails, three samples."""
    TQ.check_exact(*TQ.BIG, layout, n=3)


def test_the_geometry_of_a_display_height_that_is_no_multiple_of_8():
    TQ.check_geometry_of_a_display_height_that_is_no_multiple_of_8()


@pytest.mark.parametrize("case", [("422", 208, 104, TQ.PACKED, TQ.RGB10_F32), ("444", 176, 104, TQ.RGB10_U16, TQ.PACKED), ("422i", 192, 96, TQ.RGB10_F16, TQ.RGB10_U16)],
                         ids=["packed-then-f32", "u16-then-packed", "f16-then-u16"])
def test_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(case):
    TQ.check_short_pass_and_switching(*case)


@pytest.mark.parametrize("layout", TQ.LAYOUTS, ids=LAYOUT_IDS)
def test_failed_samples_get_cfhd_getthumbnails_status_and_zeros_among_intact_neighbours(layout):
    TQ.check_failed_samples(layout, from_device=layout in (TQ.RGB10_U16, TQ.RGB10_F32))


def test_gates():
    TQ.check_gates()


def test_kernel_names_and_times_follow_the_table():
    TQ.check_kernel_names(times_positive=True)


def test_one_pass_per_batch_several_batches_in_flight():
    TQ.check_queue_rules()


def test_the_queue_refuses_under_host_entropy():
    env = dict(os.environ, CFHD_AMD_ENTROPY="host")
    run = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import thumbnail_queue as TQ; TQ.gates_under_host_entropy()" % os.path.dirname(os.path.abspath(__file__))],
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "HOST ENTROPY REFUSED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def test_a_contiguous_float16_torch_tensor_receives_the_planes():
    """In a child process that imports torch before the library is loaded, as bench.py does: torch brings a HIP runtime of its own, and the process that runs this
    suite has long loaded the library's."""
    if importlib.util.find_spec("torch") is None: pytest.skip("no torch")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "torch"], capture_output=True, text=True, timeout=300)
    if "TORCH SEES NO DEVICE" in run.stdout: pytest.skip("torch sees no device")
    assert run.returncode == 0 and "TORCH OK" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def _torch_child():
    import torch
    if not torch.cuda.is_available(): print("TORCH SEES NO DEVICE"); return
    TQ.check_torch(torch)
    print("TORCH OK")


if __name__ == "__main__":
    _torch_child()
