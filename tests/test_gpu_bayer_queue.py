"""Bayer samples on the two queues on the MI355X (cfhd_amd_decode_batch_create_bayer, cfhd_amd_batch_create_bayer, k_inv_bayer_strip): the bodies of
tests/bayer_queue.py on the hardware.  Every picture is held byte for byte to one CFHD_DecodeSample handle fed the same samples and, where oracle/_ref is built,
to the reference decoder."""
import pytest
from cfhd_testlib import *
import bayer_queue as BQ

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("source", BQ.SOURCES)
@pytest.mark.parametrize("w,h", BQ.SHAPES)
def test_fused_last_level_equals_the_pair_equals_the_handle(w, h, source):
    if source == "ref" and not have_ref(): pytest.skip("oracle/_ref/libcfhd_ref.so is not built")
    BQ.check_fused_equals_pair_equals_handle(w, h, source)


@pytest.mark.parametrize("w,h", BQ.SHAPES)
def test_a_short_pass_is_delivered_into_device_memory_and_nothing_else_is_touched(w, h):
    BQ.check_short_pass_and_delivery(w, h)


@pytest.mark.parametrize("w,h", BQ.SHAPES)
def test_verdict_per_sample_under_both_routes(w, h):
    BQ.check_verdicts(w, h)


def test_gates():
    BQ.check_gates()


@pytest.mark.parametrize("w,h", BQ.SHAPES)
def test_frame_queue_round_trip(w, h):
    BQ.check_frame_queue_round_trip(w, h)
