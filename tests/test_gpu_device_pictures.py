"""The device-memory side of the two queues on the MI355X: cfhd_amd_decode_batch_set_device_pictures (k_dec_deliver: the pictures of a pass into device memory the caller
owns, packed or as planar u16 / f16 / f32 tensors -- the f16 layout is the hardware's convert instruction here) and cfhd_amd_batch_upload_device.  tests/device_pictures.py
has the bodies; tests/test_device_pictures_emulated.py runs them on the CPU."""
import pytest
from cfhd_testlib import *
import device_pictures as DP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,kind,w,h,out,resolution,exact", DP.PACKED_CASES, ids=[c[0] for c in DP.PACKED_CASES])
def test_packed_pictures_arrive_in_device_memory_and_nothing_else_is_touched(name, kind, w, h, out, resolution, exact):
    DP.check_packed(name, kind, w, h, out, resolution, exact)


@pytest.mark.parametrize("layout", [DP.PLANAR_U16, DP.PLANAR_F16, DP.PLANAR_F32], ids=["u16", "f16", "f32"])
@pytest.mark.parametrize("name,kind,w,h,resolution", DP.PLANAR_CASES, ids=[c[0] for c in DP.PLANAR_CASES])
def test_planar_tensors_equal_numpy_on_the_handles_words(name, kind, w, h, resolution, layout):
    DP.check_planar(name, kind, w, h, resolution, layout)


@pytest.mark.parametrize("layout", [DP.PACKED, DP.PLANAR_F16], ids=["packed", "f16"])
def test_device_memory_agrees_with_the_verdicts(layout):
    DP.check_verdicts(layout)


def test_a_short_pass_and_switching_off_leave_the_rest_alone():
    DP.check_short_pass_and_off()


def test_gates_and_the_kernel_time():
    DP.check_gates()


@pytest.mark.parametrize("name,negative_pitch", [("YUY2", False), ("RG48", False), ("YUY2 groups", False), ("YUY2", True)], ids=["yuy2", "rg48", "yuy2-groups", "yuy2-negative-pitch"])
def test_frames_from_device_memory_encode_to_the_same_samples(name, negative_pitch):
    DP.check_upload_device(name, negative_pitch)


def test_decode_to_device_pictures_then_encode_from_them():
    DP.check_chain()
