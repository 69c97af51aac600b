"""Batches of two-frame groups on the frame queue (cfhd_amd_batch_create_ex with CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP), on the GPU: the samples of two passes equal
one CFHD_EncodeSample handle's stream byte for byte (group samples, P-frame samples, sequence header), the pictures of a round trip equal CFHD_DecodeSample's (16-bit
outputs) or lie in the oracle's dither interval (8-bit 4:2:2), queued passes equal synchronous ones, and everything the issue lists is refused with NULL.  The bodies
live in tests/group_batches.py; tests/test_group_batches_emulated.py runs the same functions on the CPU.

Covered by reading, not by a test: the pass result -9 (a group sample at 80 % of width x height x bytes per pixel + 64 KB: no picture of test size reaches it) and the
refusal branches of k_dec_parse_group (the batch interface has no way to hand the decoder a damaged sample, and none was added for the test)."""
import pytest
import group_batches as GB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,name,interlaced,nframes", GB.SAMPLE_CASES)
def test_group_batch_samples_equal_the_c_abi_stream(w, h, name, interlaced, nframes):
    GB.check_samples_equal_the_c_abi_stream(w, h, name, interlaced, nframes)


@pytest.mark.parametrize("w,h,name,interlaced,nframes,flags", GB.PICTURE_CASES)
def test_group_batch_pictures(w, h, name, interlaced, nframes, flags):
    """Also the device parser against the host parser: the pictures CFHD_DecodeSample makes of the same samples go through parse_group_sample."""
    GB.check_pictures(w, h, name, interlaced, nframes, flags)


def test_group_batches_on_the_queue():
    GB.check_queue()


def test_group_batch_gates():
    GB.check_gates()
