"""One group encoder's stream on the frame queue, rate feedback included (cfhd_amd_batch_create_group_stream), on the GPU: FILMSCAN2 / FILMSCAN3 streams of two-frame
groups whose tables move inside the passes and across their boundaries, from every family of the group encoder's inputs, and MEDIUM / HIGH streams that trip the
bit-rate limiter, equal one CFHD_EncodeSample handle's stream and the reference encoder's byte for byte -- sequence header and P-frame samples included; a settled pass
and a static word take one round; group streams overlap in flight; everything the header lists is refused with NULL and a text.  The bodies live in
tests/group_stream_batches.py; tests/test_group_stream_batches_emulated.py runs the same functions on the CPU and adds the launch traces."""
import pytest
import group_stream_batches as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route,quality", G.STREAM_CASES)
def test_group_stream_equals_one_handle_and_the_reference(route, quality):
    G.check_stream(route, quality)


def test_group_stream_at_one_more_geometry():
    G.check_other_geometry()


def test_group_stream_pass_that_stands_still():
    G.check_still_pass()


@pytest.mark.parametrize("route", G.STATIC_CASES)
def test_static_word_through_the_group_stream_entry(route):
    G.check_static_word(route)


@pytest.mark.parametrize("quality", [G.MEDIUM, G.HIGH])
def test_group_stream_under_the_bit_rate_limiter(quality):
    G.check_limiter(quality)


def test_group_streams_on_the_queue():
    G.check_queue()


def test_group_stream_gates():
    G.check_gates()
    G.host_entropy_child(False)
