"""Batches of two-frame groups from RG24 / BGRA / BGRa on the frame queue (cfhd_amd_batch_create_groups) and the device coding of their subband 7, on the GPU: the
samples of two passes and CFHD_EncodeSample's equal the reference encoder's stream byte for byte, the pictures of a round trip lie within one dither step of
CFHD_DecodeSample's, queued passes equal synchronous ones, and everything the header lists is refused with NULL.  The bodies live in tests/group_batches_rgb8.py;
tests/test_group_batches_rgb8_emulated.py runs the same functions on the CPU and adds the launch trace."""
import pytest
import group_batches_rgb8 as G8
from cfhd_testlib import QUALITY_FILMSCAN1

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,w,h,nframes,flash", G8.CASES)
def test_rgb8_group_batch_samples_equal_the_reference(name, w, h, nframes, flash):
    G8.check_samples(name, w, h, nframes, flash)


@pytest.mark.parametrize("name,w,h", G8.HANDLE_CASES)
def test_rgb8_group_handle_codes_on_the_device(name, w, h):
    G8.check_handle(name, w, h)


def test_rgb8_group_handle_with_rate_feedback():
    G8.check_handle("RG24", 192, 96, quality=5, nframes=6)


@pytest.mark.parametrize("name,w,h,nframes,flash", G8.ROUNDTRIP_CASES)
def test_rgb8_group_batch_pictures(name, w, h, nframes, flash):
    G8.check_pictures(name, w, h, nframes, flash)


def test_rgb8_group_batches_on_the_queue():
    G8.check_queue()


def test_rgb8_group_batch_gates():
    G8.check_gates()
