"""Packed 4:2:2 pictures as planar Y, Cb, Cr tensors in device memory on the MI355X, on both queues: cfhd_amd_decode_batch_set_device_pictures with the YUV422_*
layouts (k_dec_deliver_yuv422 -- the bytes converted by v_cvt_f32_ubyte0 .. 3, the f16 rounding the hardware's convert instruction here) and
cfhd_amd_batch_upload_device_planar with them (k_enc_collect_yuv422 -- the f16 widening is the hardware's convert, the rounding v_rndne_f32).  tests/yuv422_planes.py
has the bodies; tests/test_yuv422_planes_emulated.py runs them on the CPU."""
import importlib.util, os, subprocess, sys
if __name__ == "__main__": import torch      # (the child of the last test: torch before anything of the library's, as bench.py has it)
import pytest
from cfhd_testlib import *
import yuv422_planes as YP
from decode_queue import FULL, HALF

pytestmark = pytest.mark.gpu
FORMAT_LAYOUTS = [(f, l) for f in YP.FORMATS for l in YP.layouts_of(f)]
FORMAT_LAYOUT_IDS = ["%s-%s" % (f, YP.LAYOUT_NAMES[l]) for f, l in FORMAT_LAYOUTS]
CHAIN = [("YUY2", YP.YUV422_U8), ("YUY2", YP.YUV422_F16), ("YUY2", YP.YUV422_F32), ("YU64", YP.YUV422_U16), ("YU64", YP.YUV422_F32)]
CHAIN_IDS = ["%s-%s" % (f, YP.LAYOUT_NAMES[l]) for f, l in CHAIN]
DELIVERIES = [("422",) + s + (FULL,) for s in YP.GEOMETRY_SHAPES + [YP.LONG32]] + [("422",) + YP.HALF_OF + (HALF,)]
DELIVERY_IDS = ["%dx%d%s" % (w, h, "-half" if r == HALF else "") for _, w, h, r in DELIVERIES]
OTHER_KINDS = [("422i", "YUY2", FULL), ("422i", "2vuy", HALF), ("groups", "YU64", FULL), ("groups", "YUY2", HALF), ("groups-i", "2vuy", FULL)]


@pytest.mark.parametrize("fmt", YP.FORMATS)
@pytest.mark.parametrize("kind,w,h,resolution", DELIVERIES, ids=DELIVERY_IDS)
def test_delivered_planes_equal_numpy_on_the_pass_own_pictures(kind, w, h, resolution, fmt):
    YP.check_delivery(kind, w, h, fmt, resolution)


@pytest.mark.parametrize("kind,fmt,resolution", OTHER_KINDS, ids=["%s-%s%s" % (k, f, "-half" if r == HALF else "") for k, f, r in OTHER_KINDS])
def test_interlaced_samples_and_groups_deliver_planes(kind, fmt, resolution):
    YP.check_delivery(kind, 192, 96, fmt, resolution)


@pytest.mark.parametrize("fmt,layout", [("YUY2", YP.YUV422_F16), ("YU64", YP.YUV422_U16)], ids=["YUY2-f16", "YU64-u16"])
def test_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(fmt, layout):
    YP.check_short_pass_and_switching(fmt, layout)


@pytest.mark.parametrize("fmt,layout", [("YUY2", YP.YUV422_U8), ("YU64", YP.YUV422_F16), ("2vuy", YP.YUV422_F32)], ids=["YUY2-u8", "YU64-f16", "2vuy-f32"])
def test_planes_agree_with_the_verdicts(fmt, layout):
    YP.check_verdicts(fmt, layout)


@pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
def test_every_element_becomes_the_word_numpy_gives(fmt, layout):
    YP.check_collection(fmt, layout)


@pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
def test_a_delivered_picture_comes_back(fmt, layout):
    YP.check_inversion(fmt, layout)


@pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
@pytest.mark.parametrize("w,h", YP.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in YP.GEOMETRY_SHAPES])
def test_runs_of_frames_at_every_geometry_and_nothing_else_touched(w, h, fmt, layout):
    YP.check_runs(fmt, w, h, layout)


@pytest.mark.parametrize("kind", YP.KIND_IDS)
def test_every_kind_of_422_batch_encodes_to_the_samples_of_the_uploaded_frames(kind):
    YP.check_kind(kind)


@pytest.mark.parametrize("kind", ["ex-2vuy-mode1", "groups-yu64"])
def test_batches_fed_float_planes_encode_to_the_same_samples(kind):
    YP.check_kind(kind, YP.YUV422_F32)


@pytest.mark.parametrize("fmt,layout", CHAIN, ids=CHAIN_IDS)
def test_decode_to_planes_then_collect_gives_the_packed_picture(fmt, layout):
    YP.check_chain(fmt, layout)


def test_decode_queue_gates():
    YP.check_decode_gates()


def test_frame_queue_gates():
    YP.check_frame_gates()


def test_the_kernel_times_and_names_follow_the_route():
    YP.check_kernel_times()


def test_a_torch_tensor_takes_the_planes_and_views_as_y_and_cbcr():
    """In a child process that imports torch before the library is loaded, as bench.py does: torch brings a HIP runtime of its own, and the process that runs this
    suite has long loaded the library's (the reference decoder's pictures also depend on whether torch was imported: cfhd_testlib.py)."""
    if importlib.util.find_spec("torch") is None: pytest.skip("no torch")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "torch"], capture_output=True, text=True, timeout=300)
    if "TORCH SEES NO DEVICE" in run.stdout: pytest.skip("torch sees no device")
    assert run.returncode == 0 and "TORCH OK" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def _torch_child():
    import torch
    if not torch.cuda.is_available(): print("TORCH SEES NO DEVICE"); return
    YP.check_torch(torch)
    print("TORCH OK")


if __name__ == "__main__":
    _torch_child()
