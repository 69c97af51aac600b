"""CPU model of the full-resolution RG48 / b64a / BGRA / BGRa decode of interlaced 4:2:2 samples (test infrastructure: nothing here is a product path).

The reference serves these outputs of an interlaced sample in two steps (Codec/decoder.c:26037 ReconstructSampleFrameYUV422ToBuffer, the switch at :26488):

1. Codec/decoder.c:22027 TransformInverseFrameToRow16u: for every band row r of each channel's level-1 wavelet, spatial.c:19803 InvertHorizontalRow16s turns
   (LL, LH) into the temporal lowpass row and (HL, HH) -- HL un-differenced -- into the temporal highpass row (the 2/6 synthesis, >> 1, saturated: the same
   arithmetic as the oracle's inv_horizontal_row), then temporal.c:7087 InvertInterlacedRow16sToRow16u writes picture row 2r = low - high and row 2r + 1 =
   low + high as 16-bit words.  Vector body (the output columns below output_width - output_width % 8 of the channel, :7137-7175): saturating difference / sum,
   clamped by the adds_epi16 / subs_epu16 pair with protect = 2047 (511 at 8-bit precision), >> 1 arithmetic, << 6 (<< 8).  Scalar tail (:7199-7227):
   (low -+ high) / 2 rounded towards zero, clamped to [0, 1023] ([0, 255]), << 6 (<< 8).  The rows are planar per picture row (Y, channel 1, channel 2);
   here they are kept as YU64 words Y0 C1 Y1 C2 (channel 1 = V, channel 2 = U), the order the reference's YU64 output and k_yu64_to_rgb16 use.
2. Codec/bayer.c:13186 ConvertRow16uToOutput -> :11916 Row16uFull2OutputFormat, its ENCODED_FORMAT_YUV_422 case without active metadata (:12180-12186):
   RGB2YUV.c:1308 ChannelYUYV16toPlanarYUV16 + :1760 PlanarYUV16toPlanarRGB16 (oracle orc_yu64_to_rgb16) at white point 16, then bayer.c:478
   ConvertLinesToOutput: RG48 / b64a take the words as they are; RGB32 (the case at :825, the unsaturated branch at :939 since the white point is 16; NEWDITHER
   is 0, :477) takes every word >> (16 - 8) and writes B, G, R, 0xff.  RGB32 rows go bottom-up (decoder.c:26395): BGRA is the flipped one, as on the
   progressive route (CFHD's BGRa is top row first).

The pyramid carries the reference's lowpass bias for the OUTPUT format (decoder.c:12240-12312, cfhd_testlib.oracle_lowpass_bias)."""
import ctypes
import numpy as np
from cfhd_testlib import Plan, PIXKIND, ENC, oracle, oracle_decode_pyramid, _oracle_levels_3_2_of_yuv422


def _sat16(x):
    return np.clip(x, -32768, 32767)


def inv_horizontal_rows(low, high):
    """spatial.c:19803 InvertHorizontalRow16s on every row of a band pair (int arrays rows x w): rows x 2w outputs (the oracle's inv_horizontal_row)."""
    lo = low.astype(np.int32); hi = high.astype(np.int32)
    h, w = lo.shape
    even = np.empty((h, w), np.int32); odd = np.empty((h, w), np.int32)
    # interior columns: saturating 16-bit steps of the vector loop
    lm, lc, lp, hc = lo[:, :-2], lo[:, 1:-1], lo[:, 2:], hi[:, 1:-1]
    e = _sat16(lm - lp); e = _sat16(e + 4) >> 3; e = _sat16(e + lc); e = _sat16(e + hc)
    o = _sat16(lp - lm); o = _sat16(o + 4) >> 3; o = _sat16(o + lc); o = _sat16(o - hc)
    even[:, 1:-1] = e >> 1; odd[:, 1:-1] = o >> 1
    # border columns (:19853-19875, :20110-20140): 32-bit sums
    even[:, 0] = (((11 * lo[:, 0] - 4 * lo[:, 1] + lo[:, 2] + 4) >> 3) + hi[:, 0]) >> 1
    odd[:, 0] = (((5 * lo[:, 0] + 4 * lo[:, 1] - lo[:, 2] + 4) >> 3) - hi[:, 0]) >> 1
    c = w - 1
    even[:, c] = (((5 * lo[:, c] + 4 * lo[:, c - 1] - lo[:, c - 2] + 4) >> 3) + hi[:, c]) >> 1
    odd[:, c] = (((11 * lo[:, c] - 4 * lo[:, c - 1] + lo[:, c - 2] + 4) >> 3) - hi[:, c]) >> 1
    out = np.empty((h, 2 * w), np.int32)
    out[:, 0::2] = _sat16(even); out[:, 1::2] = _sat16(odd)
    return out


def interlaced_row16u(low, high, precision=10):
    """temporal.c:7087 InvertInterlacedRow16sToRow16u on whole planes of temporal low / high samples (rows x output_width): (even rows, odd rows) as uint16."""
    protect = 511 if precision == 8 else 2047
    scale = 8 if precision == 8 else 6
    top = 255 if precision == 8 else 1023
    width = low.shape[1]
    post = width - width % 8
    lo = low.astype(np.int32); hi = high.astype(np.int32)
    rows = []
    for v, t in ((_sat16(lo - hi), lo - hi), (_sat16(lo + hi), lo + hi)):
        # vector body: adds_epi16(v, 0x7fff - protect), subs_epu16(., 0x7fff - protect), srai 1, slli scale
        x = _sat16(v + (0x7fff - protect)) & 0xffff
        x = np.where(x >= 0x7fff - protect, x - (0x7fff - protect), 0)
        x = (x.astype(np.uint16).view(np.int16).astype(np.int32) >> 1) << scale
        # scalar tail: C division rounds towards zero
        tail = np.clip(np.trunc(t[:, post:] / 2).astype(np.int32), 0, top) << scale
        x[:, post:] = tail
        rows.append((x & 0xffff).astype(np.uint16))
    return rows[0], rows[1]


def frame_to_yu64(plan, coeffs):
    """Decoder.c:22027 TransformInverseFrameToRow16u of a dequantized interlaced 4:2:2 pyramid (product layout, lowpass bias applied), levels 3 and 2 by the oracle:
    the picture as YU64 words (2 * band height rows of 2 * width words)."""
    work, _, _, bw, bh = _oracle_levels_3_2_of_yuv422(plan, coeffs)
    W = 2 * bw
    out = np.zeros((2 * bh, 2 * W), np.uint16)
    for c in range(3):
        w = plan.band[(c, 0, 0)]["width"]
        band = [plan.view(work, c, 0, b)[:, :w] for b in range(4)]
        low = inv_horizontal_rows(band[0], band[1])
        high = inv_horizontal_rows(band[2], band[3])
        even, odd = interlaced_row16u(low, high, plan.precision)
        sel = slice(0, None, 2) if c == 0 else (slice(1, None, 4) if c == 1 else slice(3, None, 4))
        out[0::2, sel] = even
        out[1::2, sel] = odd
    return out


def yu64_to_rgb16(yu, color_space, b64a):
    """The oracle's orc_yu64_to_rgb16 (RGB2YUV.c:1308 + :1760, bayer.c:478 at white point 16) on YU64 rows: RG48 words R, G, B or b64a words 0xffff, R, G, B."""
    O = oracle()
    rows, words = yu.shape
    W = words // 2
    yu = np.ascontiguousarray(yu)
    nw = 4 if b64a else 3
    out = np.zeros((rows, W * nw), np.uint16)
    O.orc_yu64_to_rgb16.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    O.orc_yu64_to_rgb16(yu.ctypes.data_as(ctypes.c_void_p), words, W, rows, color_space, int(bool(b64a)), out.ctypes.data_as(ctypes.c_void_p), W * nw)
    return out


def rgb16_to_rgb32(rgb, bottom_up):
    """bayer.c:825 COLOR_FORMAT_RGB32 at white point 16, no dither: every RG48 word >> 8, bytes B, G, R, 0xff; BGRA bottom row first (decoder.c:26395)."""
    rows, n = rgb.shape
    W = n // 3
    out = np.full((rows, W, 4), 0xff, np.uint8)
    px = rgb.reshape(rows, W, 3) >> 8
    out[:, :, 0] = px[:, :, 2]; out[:, :, 1] = px[:, :, 1]; out[:, :, 2] = px[:, :, 0]
    out = out.reshape(rows, 4 * W)
    return out[::-1].copy() if bottom_up else out


def model_plan(w, h, name):
    """The plan of an interlaced 4:2:2 sample decoded to `name` (its lowpass bias is the output format's)."""
    return Plan(w, h, pixkind=PIXKIND[name], enc=ENC["422"], progressive=0)


def model_decode(sample, w, h, name, color_space):
    """The whole model: an interlaced 4:2:2 sample -> YU64 words / RG48 / b64a words / BGRA / BGRa bytes, h rows (the display height)."""
    plan = model_plan(w, h, name)
    deq = oracle_decode_pyramid(sample, plan)
    yu = frame_to_yu64(plan, deq)[:h]
    if name == "YU64": return yu
    if name in ("RG48", "b64a"): return yu64_to_rgb16(yu, color_space, name == "b64a")
    return rgb16_to_rgb32(yu64_to_rgb16(yu, color_space, False), name == "BGRA")
