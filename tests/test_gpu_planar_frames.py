"""The frame queue fed from planar R, G, B tensors in device memory on the MI355X: cfhd_amd_batch_upload_device_planar (k_enc_collect -- the f16 widening is the
hardware's convert instruction here, the rounding v_rndne_f32) and cfhd_amd_batch_download_frame.  tests/planar_frames.py has the bodies;
tests/test_planar_frames_emulated.py runs them on the CPU."""
import pytest
from cfhd_testlib import *
import planar_frames as PF

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", PF.LAYOUTS, ids=PF.LAYOUT_IDS)
def test_every_element_becomes_the_word_numpy_gives(layout):
    PF.check_word_rule(layout)


@pytest.mark.parametrize("layout", [PF.PLANAR_U16, PF.PLANAR_F32], ids=["u16", "f32"])
def test_a_delivered_picture_comes_back_word_for_word(layout):
    PF.check_delivery_is_inverted(layout)


@pytest.mark.parametrize("layout", PF.LAYOUTS, ids=PF.LAYOUT_IDS)
@pytest.mark.parametrize("w,h", PF.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in PF.GEOMETRY_SHAPES])
def test_runs_of_frames_at_both_geometries_and_nothing_else_touched(w, h, layout):
    PF.check_geometry(w, h, layout)


@pytest.mark.parametrize("layout", [PF.PLANAR_U16, PF.PLANAR_F32], ids=["u16", "f32"])
@pytest.mark.parametrize("kind,mode", PF.KIND_CASES, ids=PF.KIND_IDS)
def test_every_kind_of_batch_encodes_to_the_samples_of_the_packed_frames(kind, mode, layout):
    PF.check_kind(kind, mode, layout)


def test_a_run_across_the_chunks_of_a_batch():
    PF.check_chunks()


@pytest.mark.parametrize("layout", PF.LAYOUTS, ids=PF.LAYOUT_IDS)
def test_decode_to_planar_pictures_then_encode_from_them(layout):
    PF.check_chain(layout)


def test_gates():
    PF.check_gates()


def test_download_frame_of_other_inputs():
    PF.check_download_frame_of_other_inputs()


def test_the_collect_time_follows_the_route_that_fed_the_pass():
    PF.check_kernel_time()
