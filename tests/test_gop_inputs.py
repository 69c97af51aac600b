"""Two-frame groups (CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP) from the inputs of the intra 4:2:2 encoder other than YUY2 / 2vuy, CPU side: the emulated product library
(tests/hipemu: the C ABI, GopBatch's job tables and k_fwd_gop_packed16 from the unmodified kernel source) against the compiled reference, byte for byte -- sequence
header, group samples, P-frame headers.

RG24 / BGRA / BGRa: the reference marks 8-bit RGB sources CFEncode_Temporal_Quality_32 and codes subband 7 of their groups (the lowpass band of the temporal highpass
wavelet) divided by 32 in two passes of code set 18, low bytes and then high bytes (BAND_ENCODING_LOSSLESS, Codec/encoder.c:8203, :5112), where every other source has
raw words: k_gop_quant_lowpass divides the band, the host writer codes it (vlc_encode_band_two_pass)."""
import ctypes, json, os, re, subprocess, sys
import numpy as np
import pytest
import cfhd_testlib as T
from gop_input_frames import FOURCC, INPUTS, frames, from_last_row

GOP, INTERLACED = T.ENCODING_FLAGS_2FRAME_GOP, 1
BADFORMAT = 3


def _same_stream(name, w, h, n, flags=GOP, quality=T.QUALITY_FILMSCAN1, negative_pitch=False):
    assert T.have_ref(), "oracle/_ref/libcfhd_ref.so is missing"
    data, pitch = frames(name, w, h, n)
    if negative_pitch: data, pitch = from_last_row(data, pitch, h), -pitch
    with T.emulated_product():
        mine = T.amd_encode_frames(data, pitch, w, h, FOURCC[name], flags=flags, quality=quality)
    refs = T.ref_encode_frames(data, pitch, w, h, pixfmt=FOURCC[name], flags=flags, quality=quality)
    assert [len(s) for s in mine] == [len(s) for s in refs]
    for i, (a, b) in enumerate(zip(mine, refs)):
        assert T.mask_volatile_metadata(a) == T.mask_volatile_metadata(b), "sample %d differs from the reference" % i
    assert len(mine[0]) == 40 and len(mine[2]) == 24 and min(len(mine[1]), len(mine[3])) > 4096      # sequence header, group, P-frame header, group
    return mine


# 192 x 96: whole v210 groups of 48 pixels, three tile rows; 208 x 104: a last tile of 8 of 64 columns (luma) and 4 (chroma), v210's scalar tail behind pixel 192
@pytest.mark.parametrize("w,h", [(192, 96), (208, 104)])
@pytest.mark.parametrize("name", INPUTS + ("RG64",))
def test_group_stream_equals_the_reference(name, w, h):
    mine = _same_stream(name, w, h, 4)
    assert mine[1] != mine[3]


def test_rate_feedback_follows_the_reference_from_a_16_bit_input():
    """FILMSCAN2, six frames: the quantizer tables of every group follow the size of the last key sample (derive_gop_quantization, gstate.lastgopbitcount) whatever
    the input was."""
    mine = _same_stream("YU64", 192, 96, 6, quality=5)
    assert len(set(len(s) for s in mine[1::2])) > 1


@pytest.mark.parametrize("name", ["YU64", "b64a"])
def test_negative_pitch(name):
    mine = _same_stream(name, 192, 96, 4, negative_pitch=True)
    data, pitch = frames(name, 192, 96, 4)
    with T.emulated_product():
        forward = T.amd_encode_frames(data, pitch, 192, 96, FOURCC[name], flags=GOP)
    assert [T.mask_volatile_metadata(s) for s in mine] == [T.mask_volatile_metadata(s) for s in forward]      # (the rows in memory order, as encoder.c:1957 reads them)


def test_refusals():
    """Interlaced groups are served for the inputs the interlaced intra encoder takes (YUY2 / 2vuy: the frame transform has no other loader); every other input
    answers BADFORMAT at CFHD_PrepareToEncode, and so do groups towards another encoded format than YUV 4:2:2 and from inputs that do not encode to it."""
    with T.emulated_product() as L:
        enc = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
        prep = lambda name, encoded, flags: L.CFHD_PrepareToEncode(enc, 192, 96, FOURCC.get(name) or T.fourcc(name), encoded, flags, T.QUALITY_FILMSCAN1)
        for name in INPUTS + ("RG64",):
            assert prep(name, T.ENCODED_YUV422, GOP | INTERLACED) == BADFORMAT, name
            assert prep(name, T.ENCODED_YUV422, INTERLACED) == BADFORMAT, name
        assert prep("YUY2", T.ENCODED_YUV422, GOP | INTERLACED) == 0 and prep("YUY2", T.ENCODED_YUV422, GOP) == 0
        assert prep("RG48", T.ENCODED_RGB444, GOP) == BADFORMAT and prep("b64a", T.ENCODED_RGBA4444, GOP) == BADFORMAT and prep("b64a", T.ENCODED_RGB444, GOP) == BADFORMAT
        assert prep("r210", T.ENCODED_YUV422, GOP) == BADFORMAT and prep("BYR4", T.ENCODED_BAYER, GOP) == BADFORMAT
        assert prep("YU64", T.ENCODED_YUV422, GOP) == 0 and prep("YU64", T.ENCODED_YUV422, 0) == 0
        assert prep("YU64", T.ENCODED_YUV422, GOP) == 0 and L.CFHD_PrepareToEncode(enc, 200, 96, FOURCC["YU64"], T.ENCODED_YUV422, GOP, T.QUALITY_FILMSCAN1) == BADFORMAT      # width % 16
        L.CFHD_CloseEncoder(enc)


def _child(name, flags):
    """A group encoder's reported level-1 kernel (asked before the first launch) and two calls; the name goes to stdout, the emulator's launch trace to stderr."""
    w, h = 192, 96
    data, pitch = frames(name, w, h, 2)
    with T.emulated_product() as L:
        L.cfhd_amd_encoder_kernel_name.restype = ctypes.c_char_p
        L.cfhd_amd_encoder_kernel_name.argtypes = [ctypes.c_void_p]
        enc = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
        assert L.cfhd_amd_encoder_kernel_name(enc) == b""
        assert L.CFHD_PrepareToEncode(enc, w, h, FOURCC[name], T.ENCODED_YUV422, flags, T.QUALITY_FILMSCAN1) == 0
        reported = L.cfhd_amd_encoder_kernel_name(enc).decode()
        for f in data: assert L.CFHD_EncodeSample(enc, f.ctypes.data_as(ctypes.c_void_p), pitch) == 0, T.amd_last_error()
        L.CFHD_CloseEncoder(enc)
    print("NAME " + json.dumps(reported))


@pytest.mark.parametrize("name,flags,want", [("YU64", GOP, "k_fwd_gop_packed16"), ("RG48", GOP, "k_fwd_gop_packed16"), ("YUY2", GOP, "k_fwd_yuv422"),
                                             ("YUY2", GOP | INTERLACED, "k_fwd_frame_yuv422"), ("YU64", 0, "k_fwd_packed16")])
def test_reported_level1_kernel_is_the_launched_one(name, flags, want):
    """cfhd_amd_encoder_kernel_name against the emulator's launch trace (HIPEMU_TRACE, read once per process: a fresh child), as tests/test_launch_routes_emulated.py
    does for batches: a group encoder launches the level-1 kernel it reports, once, over both frames."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(flags)], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    reported = json.loads(next(line for line in run.stdout.splitlines() if line.startswith("NAME "))[5:])
    launched = []
    for line in run.stderr.splitlines():
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid ", line)
        if m and re.match(r"k_fwd_(?!plane)", m.group(1).rsplit("::", 1)[-1]): launched.append(m.group(1).rsplit("::", 1)[-1])
    assert reported == want
    assert launched == [want] * (1 if flags & GOP else 2), launched


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[1], int(sys.argv[2]))
