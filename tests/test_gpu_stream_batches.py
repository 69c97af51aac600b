"""One encoder's stream on the frame queue, rate feedback included (cfhd_amd_batch_create_stream), on the GPU: FILMSCAN2 / FILMSCAN3 streams whose tables move inside
the passes and across their boundaries, and MEDIUM / HIGH streams that trip the bit-rate limiter, equal one CFHD_EncodeSample handle's stream and the reference
encoder's byte for byte; a settled pass and a static word take one round; stream batches overlap in flight; everything the header lists is refused with NULL and a
text.  The bodies live in tests/stream_batches.py; tests/test_stream_batches_emulated.py runs the same functions on the CPU and adds the launch traces."""
import pytest
import stream_batches as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route,quality", S.STREAM_CASES)
def test_stream_equals_one_handle_and_the_reference(route, quality):
    S.check_stream(route, quality)


def test_stream_pass_that_stands_still():
    S.check_still_pass()


@pytest.mark.parametrize("route", S.STATIC_CASES)
def test_static_word_through_the_stream_entry(route):
    S.check_static_word(route)


@pytest.mark.parametrize("quality", [S.MEDIUM, S.HIGH])
def test_stream_under_the_bit_rate_limiter(quality):
    S.check_limiter(quality)


def test_stream_batches_on_the_queue():
    S.check_queue()


def test_stream_batch_gates():
    S.check_gates()
    S.host_entropy_child(False)
