"""CPU model of a two-frame group decoded to the outputs of a 4:2:2 sample other than full-resolution 8-bit 4:2:2 (test infrastructure: nothing here is a product path).

The reference decodes a group (Codec/decoder.c:11180 DecodeSampleGroup) by inverting the three spatial wavelets and the temporal step, and then hands each frame's
level-1 wavelet to the per-output routes of an intra 4:2:2 sample.  So the model is:

1. the group pyramid by the oracle alone (cfhd_testlib.oracle_decode_group) with the lowpass bias of the REQUESTED output (group_lowpass_bias): twice the intra bias of
   that output (decoder.c:12265 `num_frames == 2 ? 48 : 24`; cfhd_testlib.oracle_lowpass_bias) except where the reference's table says otherwise -- 14, not 8, for YU64 /
   v210 of even lowpass widths (:12273-12276), and the -8 / -4 correction of RG24 / BGRA at odd widths added once to 10, not twice (:12486-12510);
2. the steps of cfhd_testlib.oracle_inverse_gop before its last level, restated here: w[5] -> w[4] lowpass, w[4] -> temporal lowpass, w[3] -> temporal highpass (the
   unprescaled wavelets through InvertSpatialQuantOverflowProtected16s, defect of its last row included), then the temporal step into the lowpass bands of w[0] / w[1];
3. each frame's level-1 wavelet through the existing intra oracle route of the output -- oracle_inverse_yu64 / _v210 / _rgb24_of_yuv422 / _rgb32_of_yuv422 /
   _rgb16_of_yuv422, the oracle_half_resolution_* family, interlaced_rgb_model for the 16-bit rows of interlaced groups -- which read the wavelet through
   FramePlanOfGroup: an intra frame plan whose level 1 is the group's w[f] and whose upper levels are empty (already inverted)."""
import numpy as np
import cfhd_testlib as T
from cfhd_testlib import PIXKIND, c_i16p
import interlaced_rgb_model as IM

FULL_PROGRESSIVE = ["YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a"]
FULL_INTERLACED = ["RG48", "b64a", "BGRA", "BGRa"]
HALF = ["YUY2", "2vuy", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a"]
HALF_INTERLACED = ["YUY2", "2vuy", "YU64", "v210", "BGRA", "BGRa", "RG48", "b64a"]      # (RG24 of interlaced samples is refused at either resolution, as for intra samples)


def served(name, width, half):
    """The product's gate (cfhd_api_decoder.inc yuv422_output_served): what a 4:2:2 sample of this width decodes to."""
    if name in ("YUY2", "2vuy"): return True
    if name in ("YU64", "RG24"): return width >= 128
    if name == "v210": return width >= 128 and (width // 2 if half else width) % 6 == 0
    if name in ("BGRA", "BGRa"): return width >= 32 and (not half or (width // 2) % 16 == 0)
    if name in ("RG48", "b64a"): return width >= (32 if half else 128)
    return False


def group_lowpass_bias(lowpass_width, name, channel):
    """What the reference decoder adds to every word of a group's raw lowpass band for output `name` (10-bit groups; Codec/decoder.c:12265-12278 even widths, :12486-12510
    the bit-serial path of odd widths, both with num_frames == 2).  Twice cfhd_testlib.oracle_lowpass_bias except for YU64 / v210 at even widths and RG24 / BGRA at odd ones."""
    if lowpass_width % 2 == 0:
        return 14 if name in ("YU64", "v210") else 48
    return 10 + ((-8 if channel == 0 else -4) if name in ("RG24", "BGRA") else 0)


def group_pyramid(sample, gp, name):
    """Dequantized group pyramid (oracle walk) carrying the lowpass bias of output `name`, per channel (odd lowpass widths: the band's words read as unsigned, as
    oracle_decode_group does)."""
    co = T.oracle_decode_group(sample, gp, lowpass_offset=0)
    for c in range(3):
        d = gp.w[(c, 5)]
        ll = gp.view(co, c, 5, 0)[:, : d["width"]]
        words = ll.view(np.uint16).astype(np.int32) if d["width"] & 1 else ll.astype(np.int32)
        ll[:] = np.minimum(words + group_lowpass_bias(d["width"], name, c), 0x7fff).astype(np.int16)
    return co


def level1_wavelets(gp, coeffs):
    """The group inverse up to the two level-1 wavelets: cfhd_testlib.oracle_inverse_gop before its last level (restated, reference defect included).  Returns the
    pyramid with each frame's level-1 lowpass band in w[0] / w[1] band 0."""
    O = T.oracle()
    work = coeffs.copy()
    def inv(c, k, dst_k, dst_b):
        d = gp.w[(c, k)]
        bands = (c_i16p * 4)(*[gp.view(work, c, k, b).ctypes.data_as(c_i16p) for b in range(4)])
        dst = gp.view(work, c, dst_k, dst_b)
        if d["prescale"] == 0:
            O.orc_inv_spatial_overflow_protected(bands, d["pitch"], d["width"], d["height"], dst.ctypes.data_as(c_i16p), gp.w[(c, dst_k)]["pitch"])
        else:
            O.orc_inv_spatial(bands, d["pitch"], d["width"], d["height"], d["prescale"], dst.ctypes.data_as(c_i16p), gp.w[(c, dst_k)]["pitch"])
    for c in range(3):
        inv(c, 5, 4, 0); inv(c, 4, 2, 0); inv(c, 3, 2, 1)
        d = gp.w[(c, 2)]
        lo = gp.view(work, c, 2, 0).astype(np.int32); hi = gp.view(work, c, 2, 1).astype(np.int32)
        even = np.clip(lo - hi, -32768, 32767) >> 1; odd = np.clip(lo + hi, -32768, 32767) >> 1
        tail = d["width"] - d["width"] % 8
        if tail < d["width"]:
            tz = lambda v: np.where(v < 0, -((-v) // 2), v // 2)
            even[:, tail:] = tz(lo[:, tail:] - hi[:, tail:]); odd[:, tail:] = tz(lo[:, tail:] + hi[:, tail:])
        gp.view(work, c, 0, 0)[:] = even.astype(np.int16); gp.view(work, c, 1, 0)[:] = odd.astype(np.int16)
    return work


class FramePlanOfGroup:
    """Frame f of a group pyramid as the intra oracle routes read a cfhd_testlib.Plan: level 1 (index 0) is the group's w[f]; levels 2 and 3 are empty bands, so the routes'
    inverse of those levels does nothing.  height: the rows of the decoded picture at full resolution (half resolution: height // 2)."""

    def __init__(self, gp, f, height):
        self.num_channels, self.precision, self.prescale = 3, 10, [0, 0, 0]
        self.width, self.height, self.pixkind, self.enc = gp.width, height, gp.pixkind, T.ENC["422"]
        self.band = {}
        for c in range(3):
            d = gp.w[(c, f)]
            for b in range(4):
                self.band[(c, 0, b)] = dict(width=d["width"], height=d["height"], pitch=d["pitch"], offset=d["offset"][b])
                for lv in (1, 2): self.band[(c, lv, b)] = dict(width=0, height=0, pitch=d["pitch"], offset=0)

    def view(self, coeffs, c, lv, b):
        d = self.band[(c, lv, b)]
        return coeffs[d["offset"]: d["offset"] + d["pitch"] * d["height"]].reshape(d["height"], d["pitch"])


def finish_frame(fp, work, name, color_space, half, interlaced):
    """One frame's level-1 wavelet (FramePlanOfGroup over the inverted group pyramid) through the intra route of output `name`.  Returns the picture as rows of bytes
    (8-bit outputs), 16-bit words (YU64, RG48, b64a) or 32-bit words (v210); RG24 at full resolution: the pair (dither 0, dither 32767) of its interval."""
    rows = fp.height
    if half:
        if name in ("YUY2", "2vuy"): return T.oracle_half_resolution(fp, work, int(name == "2vuy"))
        if name == "YU64": return T.oracle_half_resolution_yu64(fp, work)
        if name == "v210": return T.oracle_half_resolution_v210(fp, work)
        if name == "RG24": return T.oracle_half_resolution_rgb24_of_yuv422(fp, work, color_space)
        if name in ("BGRA", "BGRa"): return T.oracle_half_resolution_rgb32_of_yuv422(fp, work, name == "BGRA", color_space)
        return T.oracle_half_resolution_rgb16_of_yuv422(fp, work, name == "b64a", color_space)
    if interlaced:
        assert name in FULL_INTERLACED, name
        yu = IM.frame_to_yu64(fp, work)[:rows]
        if name in ("RG48", "b64a"): return IM.yu64_to_rgb16(yu, color_space, name == "b64a")
        return IM.rgb16_to_rgb32(IM.yu64_to_rgb16(yu, color_space, False), name == "BGRA")
    if name == "YU64": return T.oracle_inverse_yu64(fp, work)[:rows]
    if name == "v210": return T.oracle_inverse_v210(fp, work, fp.width)[:rows]
    if name == "RG24": return T.oracle_inverse_rgb24_of_yuv422(fp, work, 0, color_space), T.oracle_inverse_rgb24_of_yuv422(fp, work, 32767, color_space)
    if name in ("BGRA", "BGRa"): return T.oracle_inverse_rgb32_of_yuv422(fp, work, name == "BGRA", color_space)
    if name in ("RG48", "b64a"): return T.oracle_inverse_rgb16_of_yuv422(fp, work, name == "b64a", color_space)
    raise ValueError(name)


def model_decode_group(sample, gp, name, rows, color_space=2, half=False):
    """The whole model: a group sample -> (frame 0, frame 1) in output `name`.  rows: the picture rows the decoder reports at full resolution (the display height it
    was prepared with; half resolution gives rows // 2); color_space: 2 = 709 (the default), 1 = 601 (the group's colour space tag; frame 0 only, see below)."""
    work = level1_wavelets(gp, group_pyramid(sample, gp, name))
    # frame 1 takes the default matrix whatever the group's tag says: the reference hands it out at the P-frame sample, whose header carries no colour space tag
    return tuple(finish_frame(FramePlanOfGroup(gp, f, rows), work, name, color_space if f == 0 else 2, half, bool(gp.interlaced)) for f in range(2))


def view_output(buf, pitch, width, rows, name):
    """A decoded picture in the model's shape, cropped by the output's own pitch: `width` pixels per row (half resolution: the half width), `rows` rows."""
    buf = np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8)[: pitch * rows].reshape(rows, pitch)
    if name == "v210": return np.ascontiguousarray(buf[:, : (width // 6) * 16]).view(np.uint32)
    nbytes = {"YUY2": 2, "2vuy": 2, "RG24": 3, "BGRA": 4, "BGRa": 4, "YU64": 4, "RG48": 6, "b64a": 8}[name] * width
    px = np.ascontiguousarray(buf[:, :nbytes])
    return px.view(np.uint16) if name in ("YU64", "RG48", "b64a") else px
