"""Frames in the five Avid 4:2:2 layouts the encoder takes (avu8, av16, a106, a214, av28; Common/CFHDTypes.h:150-154), made with numpy alone from one seeded 10-bit
Y / Cr / Cb picture, with the awkward bits of every layout set on purpose -- and, for every frame, the 10-bit planes the reference's converters make of it
(Codec/frame.c:13144-13515), restated here in numpy.  Shared by tests/test_avid_inputs_emulated.py and tests/test_gpu_avid_inputs.py.  Test infrastructure only.

In memory every layout is Cb Y1 Cr Y2 per pixel pair; the planes are in the codec's channel order Y, Cr, Cb.
  avu8  bytes; plane value = byte << 2.  Every frame holds 0 and 255.
  av16  uint16 words; plane value = word >> 6.  Random low six bits in every word: a rounding shift would show.
  a106  the same arithmetic under another colour format code.
  a214  signed 2.14 words; luma ((219 y) / 16384 + 16) << 2, chroma ((224 (c + 8192)) / 16384 + 16) << 2 with C's division (toward zero), clamped to 0..1023.
        The picture rows carry the model picture; the top rows are overwritten with the whole int16 range, -1 / -16383 / 16384 and their neighbours included.
  av28  two planes: width * height / 2 bytes holding the low two bits of Cb, Y1, Cr, Y2 (bits 7-6, 5-4, 3-2, 1-0) per pixel pair, then width * height * 2 bytes
        holding their high eight bits.  Every two-bit value appears in every position of the upper plane."""
import numpy as np
import cfhd_testlib as T
from gop_input_frames import _component, from_last_row      # noqa: F401 (from_last_row: re-exported for the tests)

LAYOUTS = ("avu8", "av16", "a106", "a214", "av28")
FOURCC = {name: T.fourcc(name) for name in LAYOUTS}
COLOR_FORMAT = {"avu8": 65, "av16": 66, "av28": 67, "a214": 68, "a106": 69}      # Codec/color.h:104-108


def model_planes(w, h, seed):
    """The seeded picture: 10-bit Y (h x w), Cr and Cb (h x w/2), uint16."""
    rng = np.random.default_rng(seed)
    y = (_component(rng, w, h, seed, 0) * 1023).astype(np.uint16)
    cr = (_component(rng, w, h, seed, 1)[:, ::2] * 1023).astype(np.uint16)
    cb = (_component(rng, w, h, seed, 2)[:, ::2] * 1023).astype(np.uint16)
    return y, cr, cb


def _interleave(y, cr, cb, dtype):
    h, w = y.shape
    f = np.zeros((h, 2 * w), dtype)
    f[:, 0::4] = cb; f[:, 1::2] = y; f[:, 2::4] = cr
    return f


def c_div(a, b):
    """C's integer division of int64 arrays: toward zero."""
    return np.sign(a) * (np.abs(a) // b)


def a214_planes_of_words(words):
    """The reference's arithmetic (frame.c:13270-13292) on an (h, 2 w) int16 frame: 10-bit planes Y, Cr, Cb."""
    v = words.astype(np.int64)
    luma = (c_div(219 * v[:, 1::2], 16384) + 16) << 2
    chroma = lambda c: (c_div(224 * (c + 8192), 16384) + 16) << 2
    sat = lambda a: np.clip(a, 0, 1023).astype(np.uint16)
    return sat(luma), sat(chroma(v[:, 2::4])), sat(chroma(v[:, 0::4]))


def shift_and_division_differ(words):
    """How many samples of an a214 frame an arithmetic shift by 14 would get wrong (before the clamp hides it or not: counted on the unclamped quotient)."""
    v = words.astype(np.int64)
    y, c = 219 * v[:, 1::2], 224 * (np.concatenate([v[:, 0::4], v[:, 2::4]]) + 8192)
    return int((c_div(y, 16384) != (y >> 14)).sum() + (c_div(c, 16384) != (c >> 14)).sum())


def frame(name, w, h, seed):
    """(bytes of one frame as a uint8 array, pitch in bytes, the 10-bit planes (Y, Cr, Cb) the reference's converter makes of it)."""
    y, cr, cb = model_planes(w, h, seed)
    rng = np.random.default_rng(1000 + seed)
    if name == "avu8":
        f = _interleave(y >> 2, cr >> 2, cb >> 2, np.uint8)
        f[0, :8] = (0, 0, 0, 0, 255, 255, 255, 255); f[h - 1, -4:] = (255, 0, 255, 0)
        planes = tuple(p.astype(np.uint16) << 2 for p in (f[:, 1::2], f[:, 2::4], f[:, 0::4]))
        return f.reshape(-1).copy(), 2 * w, planes
    if name in ("av16", "a106"):
        f = (_interleave(y, cr, cb, np.uint16) << 6) | rng.integers(0, 64, (h, 2 * w)).astype(np.uint16)
        f[0, :4] = (0xffff, 0xffff, 0x003f, 0x003f)
        planes = tuple(p >> 6 for p in (f[:, 1::2], f[:, 2::4], f[:, 0::4]))
        return f.view(np.uint8).reshape(-1).copy(), 4 * w, planes
    if name == "a214":
        # the inverse of the reference's scaling, so that the model picture comes back (to within a step), with noise below the steps
        yv = (y.astype(np.int64) - 64) * 16384 // (219 * 4) + rng.integers(-9, 10, y.shape)
        cv = lambda c: (c.astype(np.int64) - 64) * 16384 // (224 * 4) - 8192 + rng.integers(-9, 10, c.shape)
        f = _interleave(yv, cv(cr), cv(cb), np.int64)
        f = np.clip(f, -32768, 32767).astype(np.int16)
        top = min(8, h // 4)                                  # the whole int16 range, luma and chroma alike
        f[:top] = rng.integers(-32768, 32768, (top, 2 * w)).astype(np.int16)
        edge = np.array([-1, -1, -16383, -16383, 16384, 16384, -32768, -32768, 32767, 32767, -8193, -8193, -8192, -1, 8191, 0, -16385, -74, 8192, 75], np.int16)
        f[0, :edge.size] = edge
        planes = a214_planes_of_words(f)
        return f.view(np.uint8).reshape(-1).copy(), 4 * w, planes
    if name == "av28":
        full = _interleave(y, cr, cb, np.uint16)              # 10-bit Cb Y1 Cr Y2
        low2 = full & 3
        low2[0, :16] = np.repeat(np.arange(4, dtype=np.uint16), 4)       # pixel pairs 0..3 of row 0: 0 0 0 0, 1 1 1 1, 2 2 2 2, 3 3 3 3
        full = (full & ~np.uint16(3)) | low2
        upper = ((low2[:, 0::4] << 6) | (low2[:, 1::4] << 4) | (low2[:, 2::4] << 2) | low2[:, 3::4]).astype(np.uint8)      # (h, w / 2)
        lower = (full >> 2).astype(np.uint8)                                                                            # (h, 2 w)
        planes = (full[:, 1::2].copy(), full[:, 2::4].copy(), full[:, 0::4].copy())
        return np.concatenate([upper.reshape(-1), lower.reshape(-1)]), 2 * w, planes      # (the pitch is ignored: frame.c:13179-13186)
    raise KeyError(name)


_cache = {}


def frames(name, w, h, n, seed=11):
    """n distinct frames (computed once per geometry, shared by the tests, never written to), their pitch and their planes."""
    key = (name, w, h, n, seed)
    if key not in _cache:
        fr = [frame(name, w, h, seed + i) for i in range(n)]
        for f, _, _ in fr: f.setflags(write=False)
        _cache[key] = ([f for f, _, _ in fr], fr[0][1], [p for _, _, p in fr])
    return _cache[key]


def words_of(name, data, w, h):
    """The a214 frame bytes as its (h, 2 w) int16 words."""
    assert name == "a214"
    return np.asarray(data).view(np.int16).reshape(h, 2 * w)
