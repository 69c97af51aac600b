"""Frames for the two-frame group encoder's inputs (tests/test_gop_inputs.py, tests/test_gpu_gop_inputs.py): distinct noise-plus-gradient pictures in every
pixel format that encodes to YUV 4:2:2, made with numpy alone.  Test infrastructure only."""
import numpy as np
import cfhd_testlib as T

FOURCC = {"YU64": T.PIX_YU64, "v210": T.PIX_V210, "RG24": T.PIX_RG24, "BGRA": T.PIX_BGRA, "BGRa": T.PIX_BGRa, "RG48": T.PIX_RG48, "b64a": T.PIX_B64A,
          "RG64": T.fourcc("RG64"), "YUY2": T.PIX_YUY2}
INPUTS = ("YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a")      # what the intra 4:2:2 encoder takes besides YUY2 / 2vuy
WORDS16 = {"RG48": 3, "b64a": 4, "RG64": 4}
BYTES8 = {"RG24": 3, "BGRA": 4, "BGRa": 4}


def _component(rng, w, h, seed, k):
    y, x = np.mgrid[0:h, 0:w]
    v = 0.5 + 0.35 * np.sin(x / (17.0 + 5 * k) + seed) * np.cos(y / (11.0 + 3 * k)) + 0.1 * ((x + 2 * y + 7 * seed) % 64) / 64.0 + rng.normal(0, 0.02, (h, w))
    return np.clip(v, 0, 1)


def frame(name, w, h, seed):
    """(bytes of one frame as a uint8 array, pitch in bytes)."""
    if name == "v210":
        f = T.synth_v210(w, h, seed)
        return f[0], f[1]
    if name == "YUY2": return T.synth_yuy2(w, h, seed)
    rng = np.random.default_rng(seed)
    if name == "YU64":                                  # words Y0 C1 Y1 C2
        f = np.zeros((h, w * 2), np.uint16)
        f[:, 0::2] = (_component(rng, w, h, seed, 0) * 65535).astype(np.uint16)
        f[:, 1::4] = (_component(rng, w, h, seed, 1)[:, ::2] * 65535).astype(np.uint16)
        f[:, 3::4] = (_component(rng, w, h, seed, 2)[:, ::2] * 65535).astype(np.uint16)
        return f.view(np.uint8).reshape(-1).copy(), w * 4
    if name in BYTES8:
        n = BYTES8[name]
        f = np.stack([(_component(rng, w, h, seed, k) * 255).astype(np.uint8) for k in range(n)], axis=2)
        return f.reshape(-1).copy(), w * n
    n = WORDS16[name]
    f = np.stack([(_component(rng, w, h, seed, k) * 65535).astype(np.uint16) for k in range(n)], axis=2)
    return np.ascontiguousarray(f).view(np.uint8).reshape(-1).copy(), w * n * 2


_cache = {}


def frames(name, w, h, n, seed=5):
    """n distinct frames (computed once per geometry, shared by the tests, never written to) and their pitch."""
    key = (name, w, h, n, seed)
    if key not in _cache:
        fr = [frame(name, w, h, seed + i) for i in range(n)]
        for f, _ in fr: f.setflags(write=False)
        _cache[key] = ([f for f, _ in fr], fr[0][1])
    return _cache[key]


def from_last_row(data, pitch, h):
    """Views of the same buffers that start at their last row: what a caller hands over together with the pitch negated (Codec/encoder.c:1957 steps back to the
    first byte and reads the rows in memory order)."""
    return [np.asarray(f)[(h - 1) * pitch:] for f in data]
