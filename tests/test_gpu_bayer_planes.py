"""BYR4 mosaics as four planar component tensors in device memory on the MI355X, on both queues: cfhd_amd_decode_batch_set_device_pictures with the BAYER_* layouts
(k_dec_deliver_bayer -- the f16 rounding is the hardware's convert instruction here) and cfhd_amd_batch_upload_device_planar with them (k_enc_collect_bayer -- the f16
widening is the hardware's convert, the rounding v_rndne_f32).  tests/bayer_planes.py has the bodies; tests/test_bayer_planes_emulated.py runs them on the CPU."""
import pytest
from cfhd_testlib import *
import bayer_planes as BP

pytestmark = pytest.mark.gpu
TWO = [BP.BAYER_U16, BP.BAYER_F32]


@pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
@pytest.mark.parametrize("w,h", BP.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in BP.GEOMETRY_SHAPES])
def test_delivered_planes_equal_numpy_on_the_handles_mosaics(w, h, layout):
    BP.check_delivery(w, h, layout)


@pytest.mark.parametrize("layout", [BP.BAYER_F16, BP.BAYER_F32], ids=["f16", "f32"])
def test_a_short_pass_touches_nothing_else_and_packed_and_null_switch_back(layout):
    BP.check_short_pass_and_switching(layout)


@pytest.mark.parametrize("layout", [BP.BAYER_U16, BP.BAYER_F16], ids=["u16", "f16"])
def test_planes_agree_with_the_verdicts(layout):
    BP.check_verdicts(layout)


@pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
def test_every_element_becomes_the_word_numpy_gives(layout):
    BP.check_collection(layout)


@pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
def test_a_delivered_mosaic_comes_back(layout):
    BP.check_inversion(layout)


@pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
@pytest.mark.parametrize("w,h", BP.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in BP.GEOMETRY_SHAPES])
def test_runs_of_frames_at_every_geometry_and_nothing_else_touched(w, h, layout):
    BP.check_runs(w, h, layout)


@pytest.mark.parametrize("layout", TWO, ids=["u16", "f32"])
@pytest.mark.parametrize("kind", BP.KIND_IDS)
def test_every_kind_of_byr4_batch_encodes_to_the_samples_of_the_uploaded_mosaics(kind, layout):
    BP.check_kind(kind, layout)


@pytest.mark.parametrize("layout", TWO, ids=["u16", "f32"])
def test_decode_to_planes_then_encode_from_them(layout):
    BP.check_chain(layout)


def test_decode_queue_gates():
    BP.check_decode_gates()


def test_frame_queue_gates():
    BP.check_frame_gates()


def test_the_kernel_times_and_names_follow_the_route():
    BP.check_kernel_times()
