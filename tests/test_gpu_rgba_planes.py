"""Pictures that carry alpha as planar R, G, B, A tensors in device memory on the MI355X, on both queues: cfhd_amd_decode_batch_set_device_pictures with the RGBA_*
layouts (k_dec_deliver_rgba -- the components separated by v_perm_b32, the bytes converted by v_cvt_f32_ubyte0 .. 3, the f16 rounding the hardware's convert
instruction here) and cfhd_amd_batch_upload_device_planar with them (k_enc_collect_rgba -- the f16 widening is the hardware's convert, the rounding v_rndne_f32).
tests/rgba_planes.py has the bodies; tests/test_rgba_planes_emulated.py runs them on the CPU."""
import importlib.util, os, subprocess, sys
if __name__ == "__main__": import torch      # (the child of the last test: torch before anything of the library's, as bench.py has it)
import pytest
from cfhd_testlib import *
import rgba_planes as RP

pytestmark = pytest.mark.gpu
FORMAT_LAYOUTS = [(f, l) for f in RP.FORMATS for l in RP.layouts_of(f)]
FORMAT_LAYOUT_IDS = ["%s-%s" % (f, RP.LAYOUT_NAMES[l]) for f, l in FORMAT_LAYOUTS]
CHAIN = [("b64a", RP.RGBA_U16), ("b64a", RP.RGBA_F16), ("b64a", RP.RGBA_F32), ("BGRA", RP.RGBA_U8), ("BGRA", RP.RGBA_F16), ("BGRa", RP.RGBA_F32)]
CHAIN_IDS = ["%s-%s" % (f, RP.LAYOUT_NAMES[l]) for f, l in CHAIN]


@pytest.mark.parametrize("name", RP.DECODE_IDS)
def test_delivered_planes_equal_numpy_on_the_pass_own_pictures(name):
    RP.check_delivery(name)


@pytest.mark.parametrize("fmt,layout", [("b64a", RP.RGBA_F16), ("BGRA", RP.RGBA_U8)], ids=["b64a-f16", "BGRA-u8"])
def test_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(fmt, layout):
    RP.check_short_pass_and_switching(fmt, layout)


@pytest.mark.parametrize("fmt,layout", [("b64a", RP.RGBA_F16), ("BGRA", RP.RGBA_U8), ("BGRa", RP.RGBA_F32)], ids=["b64a-f16", "BGRA-u8", "BGRa-f32"])
def test_planes_agree_with_the_verdicts(fmt, layout):
    RP.check_verdicts(fmt, layout)


@pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
def test_every_element_becomes_the_word_numpy_gives(fmt, layout):
    RP.check_collection(fmt, layout)


@pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
def test_a_delivered_picture_comes_back(fmt, layout):
    RP.check_inversion(fmt, layout)


@pytest.mark.parametrize("kind", RP.KIND_IDS)
def test_every_kind_of_batch_takes_the_planes_and_encodes_to_the_samples_of_the_uploaded_frames(kind):
    RP.check_kind(kind)


def test_a_stream_fed_planes_for_two_passes_equals_the_stream_fed_packed_frames():
    RP.check_stream()


@pytest.mark.parametrize("fmt,layout", CHAIN, ids=CHAIN_IDS)
def test_decode_to_planes_then_collect_gives_the_packed_picture(fmt, layout):
    RP.check_chain(fmt, layout)


def test_decode_queue_gates():
    RP.check_decode_gates()


def test_frame_queue_gates():
    RP.check_frame_gates()


def test_the_kernel_times_and_names_follow_the_route():
    RP.check_kernel_times()


def test_a_torch_tensor_takes_the_four_planes_and_gives_them_back():
    """In a child process that imports torch before the library is loaded, as bench.py does: torch brings a HIP runtime of its own, and the process that runs this
    suite has long loaded the library's."""
    if importlib.util.find_spec("torch") is None: pytest.skip("no torch")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "torch"], capture_output=True, text=True, timeout=300)
    if "TORCH SEES NO DEVICE" in run.stdout: pytest.skip("torch sees no device")
    assert run.returncode == 0 and "TORCH OK" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def _torch_child():
    import torch
    if not torch.cuda.is_available(): print("TORCH SEES NO DEVICE"); return
    RP.check_torch(torch)
    print("TORCH OK")


if __name__ == "__main__":
    _torch_child()
