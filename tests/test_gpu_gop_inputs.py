"""Two-frame groups from the inputs of the intra 4:2:2 encoder other than YUY2 / 2vuy, on the GPU through the C ABI: CFHD_EncodeSample with
CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP gives the reference encoder's samples byte for byte (level 1 of both frames: k_fwd_gop_packed16), and the product decodes its own
stream to the pictures it decodes the reference's stream to.

RG24 / BGRA / BGRa: subband 7 of their groups is divided by 32 on the device (k_gop_quant_lowpass) and coded in two passes by the host writer, as the reference codes
it (BAND_ENCODING_LOSSLESS: tests/test_gop_inputs.py); the decoder reads that band back on the host."""
import ctypes
import numpy as np
import pytest
import cfhd_testlib as T
from gop_input_frames import FOURCC, INPUTS, frames

pytestmark = pytest.mark.gpu
GOP = T.ENCODING_FLAGS_2FRAME_GOP
_streams = {}


def _streams_of(name, w, h, quality=T.QUALITY_FILMSCAN1, n=4):
    """(product's samples, reference's samples) of one case, encoded once and shared."""
    key = (name, w, h, quality, n)
    if key not in _streams:
        assert T.have_ref(), "oracle/_ref/libcfhd_ref.so is missing"
        data, pitch = frames(name, w, h, n)
        mine = T.amd_encode_frames(data, pitch, w, h, FOURCC[name], flags=GOP, quality=quality)
        box = {}
        def leg():
            box["refs"] = T.ref_encode_frames(data, pitch, w, h, pixfmt=FOURCC[name], flags=GOP, quality=quality)
            return [T.mask_volatile_metadata(a) for a in mine] == [T.mask_volatile_metadata(b) for b in box["refs"]] or "sizes %s vs reference %s" % (
                [len(s) for s in mine], [len(s) for s in box["refs"]])
        T.reference_leg(leg, 2, "group encode from %s" % name)
        _streams[key] = (mine, box["refs"])
    return _streams[key]


@pytest.mark.parametrize("w,h", [(192, 96), (320, 240), (208, 104)])
@pytest.mark.parametrize("name", INPUTS + ("RG64",))
def test_group_stream_equals_the_reference(name, w, h):
    mine, refs = _streams_of(name, w, h)
    assert [len(s) for s in mine] == [len(s) for s in refs]
    for i, (a, b) in enumerate(zip(mine, refs)):
        assert T.mask_volatile_metadata(a) == T.mask_volatile_metadata(b), "sample %d differs from the reference" % i
    assert len(mine[0]) == 40 and len(mine[2]) == 24 and mine[1] != mine[3]


def test_rate_feedback_follows_the_reference_from_a_16_bit_input():
    mine, refs = _streams_of("YU64", 192, 96, quality=5, n=6)
    assert [T.mask_volatile_metadata(a) for a in mine] == [T.mask_volatile_metadata(b) for b in refs]
    assert len(set(len(s) for s in mine[1::2])) > 1


def _decode_stream(samples, w, h):
    """Every picture of a stream of groups through one decoder handle prepared on the first group, to YUY2 at full resolution (the dither bits follow the call
    count: same calls, same bits)."""
    L = T.product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
    sb = ctypes.create_string_buffer(samples[1], len(samples[1]))
    assert L.CFHD_PrepareToDecode(dec, 0, 0, T.PIX_YUY2, 1, 0, sb, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
    assert (aw.value, ah.value) == (w, h)
    out = []
    for s in samples[1:]:                                # (samples[0] is the sequence header)
        sb = ctypes.create_string_buffer(s, len(s)); pic = np.zeros(w * 2 * h, np.uint8)
        rc = L.CFHD_DecodeSample(dec, sb, len(s), pic.ctypes.data_as(ctypes.c_void_p), w * 2)
        assert rc == 0, "CFHD_DecodeSample -> %d (%s)" % (rc, T.amd_last_error())
        out.append(pic)
    L.CFHD_CloseDecoder(dec)
    return out


@pytest.mark.parametrize("name", INPUTS)
def test_round_trip_equals_the_decode_of_the_reference_stream(name):
    w, h = 192, 96
    mine, refs = _streams_of(name, w, h)
    a, b = _decode_stream(mine, w, h), _decode_stream(refs, w, h)
    assert len(a) == 3                                  # group, P-frame header, group: frames 0, 1, 2 (the last frame would come with a fifth call)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "picture %d" % i


def test_level1_kernel_of_a_group_encoder():
    L = T.product()
    L.cfhd_amd_encoder_kernel_name.restype = ctypes.c_char_p
    L.cfhd_amd_encoder_kernel_name.argtypes = [ctypes.c_void_p]
    enc = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
    for name, flags, want in (("YU64", GOP, b"k_fwd_gop_packed16"), ("b64a", GOP, b"k_fwd_gop_packed16"), ("YUY2", GOP, b"k_fwd_yuv422"), ("YUY2", GOP | 1, b"k_fwd_frame_yuv422")):
        assert L.CFHD_PrepareToEncode(enc, 192, 96, FOURCC[name], T.ENCODED_YUV422, flags, T.QUALITY_FILMSCAN1) == 0
        assert L.cfhd_amd_encoder_kernel_name(enc) == want
    L.CFHD_CloseEncoder(enc)
