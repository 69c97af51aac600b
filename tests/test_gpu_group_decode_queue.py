"""The decode queue for streams of two-frame groups on the MI355X (cfhd_amd_decode_batch_create_groups): group streams of the reference's encoder and of the
product's, 4 groups a pass, against one CFHD_DecodeSample handle fed the same samples (tests/group_decode_queue.py has the bodies;
tests/test_group_decode_queue_emulated.py runs them on the CPU)."""
import os, subprocess, sys
import pytest
from cfhd_testlib import *
import group_decode_queue as GQ

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")
SOURCES = [pytest.param("ref", marks=needs_ref), "amd"]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("interlaced,w,h,out,resolution", GQ.EXACT_CASES)
def test_foreign_groups_decode_to_the_handles_pictures(interlaced, w, h, out, resolution, source):
    GQ.check_foreign_exact(interlaced, w, h, out, resolution, source)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("interlaced,w,h,out,exact_out", GQ.DITHER_CASES)
def test_dithered_outputs_stay_within_one_step_of_the_handle(interlaced, w, h, out, exact_out, source):
    GQ.check_foreign_dithered(interlaced, w, h, out, exact_out, source)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("pix,w,h", GQ.TWO_PASS_CASES)
def test_the_two_pass_band_is_decoded_on_the_device(pix, w, h, source):
    GQ.check_two_pass_on_the_device(pix, w, h, source)


@pytest.mark.parametrize("source", SOURCES)
def test_one_pass_mixes_qualities(source):
    GQ.check_mixed_qualities(source)


@pytest.mark.parametrize("source", SOURCES)
def test_one_pass_mixes_raw_word_and_two_pass_groups(source):
    GQ.check_mixed_band_kinds(source)


@pytest.mark.parametrize("source", SOURCES)
def test_ingest_from_plain_registered_and_device_memory(source):
    GQ.check_ingest(source)


@pytest.mark.parametrize("source", SOURCES)
def test_a_short_pass_leaves_the_rest_alone(source):
    GQ.check_short_pass(source)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind,follower_kind", [(k, GQ.FOLLOWER_KINDS[i % 3]) for i, k in enumerate(GQ.VERDICT_KINDS)])
def test_verdict_per_pair(kind, follower_kind, source):
    GQ.check_verdicts(kind, follower_kind, source)


def test_a_sequence_header_passed_as_a_sample_has_a_zero_picture():
    GQ.check_sequence_header_as_a_sample()


@pytest.mark.parametrize("source", SOURCES)
def test_two_group_batches_in_flight(source):
    GQ.check_queue(source)


def test_gates():
    GQ.check_gates()


def test_gate_under_host_entropy():
    env = dict(os.environ, CFHD_AMD_ENTROPY="host")
    code = "import sys; sys.path.insert(0, %r); import group_decode_queue as GQ; GQ.gates_under_host_entropy()" % os.path.dirname(os.path.abspath(__file__))
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "HOST ENTROPY REFUSED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
