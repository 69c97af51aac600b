"""The decode queue on the MI355X (cfhd_amd_decode_batch_*): samples of the reference's encoder and of the product's, 8 or 17 a pass, against one CFHD_DecodeSample
handle fed the same samples (tests/decode_queue.py has the bodies; tests/test_decode_queue_emulated.py runs them on the CPU)."""
import os, subprocess, sys
import pytest
from cfhd_testlib import *
import decode_queue as DQ

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")
SOURCES = [pytest.param("ref", marks=needs_ref), "amd"]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind,w,h,out,resolution", DQ.EXACT_CASES)
def test_foreign_samples_decode_to_the_handles_pictures(kind, w, h, out, resolution, source):
    DQ.check_foreign_exact(kind, w, h, out, resolution, source)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind,w,h,out,exact_out", DQ.DITHER_CASES)
def test_dithered_outputs_stay_within_one_step_of_the_handle(kind, w, h, out, exact_out, source):
    DQ.check_foreign_dithered(kind, w, h, out, exact_out, source)


@pytest.mark.parametrize("source", SOURCES)
def test_one_pass_mixes_qualities(source):
    DQ.check_mixed_qualities(source)


@needs_ref
def test_ingest_from_plain_registered_and_device_memory():
    DQ.check_ingest()


@needs_ref
def test_short_samples_after_long_ones():
    DQ.check_short_samples_after_long_ones()


@needs_ref
def test_a_short_pass_leaves_the_rest_alone():
    DQ.check_short_pass_leaves_the_rest_alone()


@needs_ref
@pytest.mark.parametrize("kind", DQ.VERDICT_KINDS)
def test_verdict_per_sample(kind):
    DQ.check_verdicts(kind)


@needs_ref
def test_two_decode_batches_in_flight():
    DQ.check_queue()


def test_gates():
    DQ.check_gates()


def test_gate_under_host_entropy():
    env = dict(os.environ, CFHD_AMD_ENTROPY="host")
    code = "import sys; sys.path.insert(0, %r); import decode_queue as DQ; DQ.gates_under_host_entropy()" % os.path.dirname(os.path.abspath(__file__))
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "HOST ENTROPY REFUSED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
