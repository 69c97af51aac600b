"""The YU64 picture of an RGB 4:4:4 or RGBA 4:4:4:4 sample as a pure function of its RG48 picture: a numpy float32 model of the reference decoder's conversion
(ReconstructSampleFrameRGB444ToBuffer -> TransformInverseRGB444ToYU64 -> ConvertPlanarRGB16uToPackedYU64, Codec/decoder.c:26874, Codec/wavelet.c:4515,
Codec/convert.c:7312; the arithmetic is the scalar loop at convert.c:7841-7864, restated).

For RG48 words r, g, b (0 .. 65535), pixels (2 k, 2 k + 1) of a row a pair; every product and sum IEEE binary32, evaluated left to right as (cr * R + cg * G) + cb * B;
every coefficient (float)c * 64.0f; the conversion to int truncates toward zero; >> on the int is arithmetic:
    Y(x)  = sat16(((int)(yr r + yg g + yb b) >> 6) + 4096)
    Cb(k) = sat16(((int)(ur (r0 + r1) + ug (g0 + g1) + ub (b0 + b1)) >> 7) + 32768), Cr(k) the same with the v row; the sums are converted to float once
    sat16 clamps to [0, 65535]
4096 is added under both matrices, the video-systems one too: bright pixels saturate there, as they do in the reference.
The matrix rows (y; u; v) follow bit 2 (value 4) of the sample's colour-space tag (tag 91; absent: 0).  The 601 bit has no effect on these samples.

tests/test_rgb_as_yuv_model_vs_ref.py holds the model to the reference word for word; tests/rgb_as_yuv.py holds k_dec_deliver_rgb_as_yuv to the model.
Test infrastructure only."""
import numpy as np

F = np.float32
MATRIX_CG = ((0.183, 0.614, 0.062), (-0.101, -0.338, 0.439), (0.439, -0.399, -0.040))      # the tag absent or bit 2 clear
MATRIX_VS = ((0.213, 0.715, 0.072), (-0.117, -0.394, 0.511), (0.511, -0.464, -0.047))      # bit 2 set: "video systems"


def matrix_of(tag):
    """The rows (y; u; v) as the float32 coefficients the arithmetic uses: (float)c * 64.0f."""
    rows = MATRIX_VS if (tag & 4) else MATRIX_CG
    return [[F(c) * F(64.0) for c in row] for row in rows]


def _dot(row, r, g, b):
    s = (row[0] * r + row[1] * g) + row[2] * b
    assert s.dtype == np.float32
    return s.astype(np.int32)                                   # (numpy truncates toward zero; every value is far inside int32)


def _sat16(v):
    return np.clip(v, 0, 65535).astype(np.uint16)


def yuv_of_rg48(picture, w, h, tag=0):
    """An RG48 picture (h rows of 6 w bytes, w even) -> (Y uint16 [h, w], Cb uint16 [h, w / 2], Cr uint16 [h, w / 2])."""
    assert w % 2 == 0
    px = np.ascontiguousarray(picture).reshape(-1).view(np.uint16).reshape(h, w, 3).astype(np.int32)
    m = matrix_of(tag)
    r, g, b = (px[:, :, c].astype(F) for c in range(3))
    y = _sat16((_dot(m[0], r, g, b) >> 6) + 4096)
    pairs = px[:, 0::2, :] + px[:, 1::2, :]
    rs, gs, bs = (pairs[:, :, c].astype(F) for c in range(3))
    cb = _sat16((_dot(m[1], rs, gs, bs) >> 7) + 32768)
    cr = _sat16((_dot(m[2], rs, gs, bs) >> 7) + 32768)
    return y, cb, cr


def yu64_of_rg48(picture, w, h, tag=0):
    """... as the packed YU64 picture: uint8 [h, 4 w], the words Y0 Cr Y1 Cb of every pair."""
    y, cb, cr = yuv_of_rg48(picture, w, h, tag)
    out = np.empty((h, w // 2, 4), np.uint16)
    out[:, :, 0] = y[:, 0::2]; out[:, :, 1] = cr; out[:, :, 2] = y[:, 1::2]; out[:, :, 3] = cb
    return out.reshape(h, 2 * w).view(np.uint8)


def planes_of_yu64(yu64, w, h):
    """The packed YU64 picture back as (Y, Cb, Cr)."""
    words = np.ascontiguousarray(yu64).reshape(-1).view(np.uint16).reshape(h, w // 2, 4)
    y = np.empty((h, w), np.uint16); y[:, 0::2] = words[:, :, 0]; y[:, 1::2] = words[:, :, 2]
    return y, np.ascontiguousarray(words[:, :, 3]), np.ascontiguousarray(words[:, :, 1])


def _tag_offset(sample):
    """The offset of the sample's colour-space tag-value pair (tag 91, written as the optional tag -91: the bytes FF A5 vv vv) in the header in front of the first
    band, or None.  The walk skips the payloads of the chunks in its way, as cfhd_testlib.first_metadata_chunk does."""
    s, pos = bytes(sample), 0
    while pos + 4 <= len(s):
        tag = int.from_bytes(s[pos: pos + 2], "big", signed=True); val = int.from_bytes(s[pos + 2: pos + 4], "big")
        t = -tag if tag < 0 else tag
        if t == 91: return pos
        if t in (55, 56): return None                           # (TAG_BAND_HEADER / a band's code stream: the header is over)
        pos += 4
        if t == 2: pos += 4 * val
        elif t & 0x4000: pos += 4 * val
    return None


def color_space_tag(sample):
    """The value of the sample's colour-space tag, or None where it has none."""
    at = _tag_offset(sample)
    return None if at is None else int.from_bytes(bytes(sample[at + 2: at + 4]), "big")


def with_tag(sample, value):
    """The sample with the value of its colour-space tag replaced (the tag has to be there)."""
    at = _tag_offset(sample)
    assert at is not None, "the sample carries no colour-space tag"
    s = bytearray(sample); s[at + 2: at + 4] = int(value).to_bytes(2, "big")
    return bytes(s)
