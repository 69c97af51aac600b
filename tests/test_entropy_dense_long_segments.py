"""Long segments for the bands k_ent_count counts densely (cfhd_entropy_jobs.h EntSegRule: level 1 without block lists, level 2, level 3): the GPU entropy stage under
the CPU emulation of tests/hipemu writes the same sample, byte for byte, for every combination of level-2 and level-3 segment length in {1024, 2048, 4096, 8192} and for
dense level-1 segments of 1024 and 4096 -- and that sample is the product's host writer's.

Shapes: 512 x 272 YUY2 -- luma level 2 has 8704 coefficients (4096 + 4096 + 512), chroma level 2 4352 (4096 + 256), luma level 3 2176, chroma level 3 1088 (shorter than
one long segment); its level-1 bands go through k_ent_count_blocks with ENT_SEG_L1, as in the product.  256 x 136 RG48 (RGB 4:4:4) for dense level-1 bands of 8704."""
import ctypes, itertools, os
import numpy as np
import pytest
from cfhd_testlib import (ROOT, PRODUCT_DIR, PIXKIND, ENC, COLOR_FORMAT_YUYV, COLOR_FORMAT_RG48, PIX_RG48, Plan, _build_once, c_i16p, c_u8p, oracle_forward_yuv422,
                          oracle_forward_planes, rg48_planes, p8, p16, product_write_sample_host, synth_yuy2)

SO = os.path.join(ROOT, "tests", "_build", "libcfhd_emu_dense_long_segments.so")
_lib = None
META = b"GUID\x10\x00\x00G" + bytes(range(16))
LENGTHS = (1024, 2048, 4096, 8192)
W, H = 512, 272          # YUY2
RW, RH = 256, 136        # RG48


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(PRODUCT_DIR, "csrc"); hipemu = os.path.join(ROOT, "tests", "hipemu")
        src = os.path.join(hipemu, "emu_dense_long_segments.cpp")
        host = [os.path.join(csrc, f) for f in ("cfhd_tables.cpp", "cfhd_bitstream.cpp", "cfhd_gop.cpp")]
        deps = [src, os.path.join(hipemu, "hip_emu.h"), os.path.join(hipemu, "cfhd_gfx950.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".cpp"))]
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        _build_once(SO, ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I" + hipemu, "-I" + csrc, src] + host, deps)
        L = ctypes.CDLL(SO)
        L.emu_dense_long_encode.restype = ctypes.c_long
        L.emu_dense_long_encode.argtypes = [ctypes.c_int] * 7 + [ctypes.c_uint, c_i16p, c_u8p, ctypes.c_size_t, c_u8p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_long)]
        _lib = L
    return _lib


def encode(plan, coeffs, l1_dense=1024, l2=1024, l3=1024, l1_lists=4096, use_lists=None, interlaced=0, input_format=COLOR_FORMAT_YUYV, color_space=2):
    """-> (sample, stats): see emu_dense_long_encode.  use_lists defaults to what the product does: block lists for progressive 4:2:2 frames."""
    if use_lists is None: use_lists = int(plan.enc == ENC["422"] and not interlaced)
    out = np.zeros(plan.width * plan.height * 8 + 65536, dtype=np.uint8)
    m = np.frombuffer(META, dtype=np.uint8).copy()
    stats = (ctypes.c_long * 9)()
    lens = (ctypes.c_int * 4)(l1_lists, l1_dense, l2, l3)
    n = lib().emu_dense_long_encode(plan.width, plan.height, plan.pixkind, plan.enc, plan.quality, input_format, color_space, 1, p16(coeffs), p8(m), len(META), p8(out), out.size,
                                    interlaced, lens, use_lists, stats)
    assert n > 0, n
    return bytes(out[:n]), list(stats)


def differs(got, base):
    if got == base: return None
    first = next(k for k in range(min(len(got), len(base))) if got[k] != base[k]) if len(got) == len(base) else -1
    return "%d bytes against %d, first difference at %d" % (len(got), len(base), first)


def check_level23_lengths(plan, coeffs, want=None):
    """Every combination of level-2 and level-3 length against the sample of 1024 everywhere (equal to `want` when given).  Returns that sample and the stats by (l2, l3)."""
    base, st = encode(plan, coeffs)
    assert st[7] == 1024
    if want is not None: assert differs(base, want) is None, differs(base, want)
    stats = {(1024, 1024): st}
    for l2, l3 in itertools.product(LENGTHS, LENGTHS):
        if (l2, l3) == (1024, 1024): continue
        got, st = encode(plan, coeffs, l2=l2, l3=l3)
        assert st[7] == min(max(l2, l3), 8704)               # (the level-2 / level-3 bands did get those segments: the longest band has 8704 coefficients)
        d = differs(got, base)
        assert d is None, "l2=%d l3=%d: %s" % (l2, l3, d)
        stats[(l2, l3)] = st
    return base, stats


def yuy2_plan_and_coeffs(seed):
    frame, pitch = synth_yuy2(W, H, seed)
    plan = Plan(W, H)
    return plan, oracle_forward_yuv422(plan, frame, pitch)


def upper_views(plan, coeffs, levels=(1, 2)):
    for c in range(3):
        for lv in levels:
            for b in (1, 2, 3):
                yield c, lv, plan.band[(c, lv, b)], plan.view(coeffs, c, lv, b)


def test_band_sizes_give_every_case():
    plan = Plan(W, H)
    n = lambda c, lv: plan.band[(c, lv, 1)]["pitch"] * plan.band[(c, lv, 1)]["height"]
    assert (n(0, 1), n(1, 1), n(0, 2), n(1, 2)) == (8704, 4352, 2176, 1088)
    rplan = Plan(RW, RH, pixkind=PIXKIND["RG48"], enc=ENC["444"])
    d = rplan.band[(0, 0, 1)]
    assert d["pitch"] * d["height"] == 8704


def test_level2_level3_lengths_synthetic_picture():
    plan, coeffs = yuy2_plan_and_coeffs(3)
    check_level23_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META))


def test_level2_level3_lengths_noise_leaves_the_lds_window():
    """Noise of large values in the bands of levels 2 and 3: a level-3 segment of 2048 coefficients and more codes into more than ENT_LDS_WORDS words, so its code words go
    to the payload with global atomics (k_ent_emit, use_lds false) and its neighbours cannot merge the shared words."""
    plan, coeffs = yuy2_plan_and_coeffs(1)
    rng = np.random.default_rng(7)
    for c, lv, d, v in upper_views(plan, coeffs):
        shape = (d["height"], d["width"])
        v[:, : d["width"]] = rng.integers(1, 901, size=shape) * rng.choice([-1, 1], size=shape)
    _, stats = check_level23_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META))
    assert stats[(1024, 1024)][6] == 0
    for l2, l3 in stats:
        if l3 >= 2048: assert stats[(l2, l3)][6] > 0 and stats[(l2, l3)][3] > 32 * 1024, (l2, l3, stats[(l2, l3)])      # long level-3 segments took the atomic path


def test_level2_level3_lengths_flat_picture_with_impulses():
    """Isolated nonzeros in empty bands: zero runs of 3072 and more inside one level-2 segment and across its windows of 1024 (past the run tables: the token takes
    k_ent_emit's table walk), runs that cross segments, tokens on the first and last coefficient of windows, segments and bands, values beyond +-1023."""
    plan, coeffs = yuy2_plan_and_coeffs(2)
    vals = [5000, -7000, 1023, -1024, 2, -1, 1500, -3000, 700, -2000, 4, 9]
    found = False
    for c, lv, d, v in upper_views(plan, coeffs):
        assert d["pitch"] == d["width"]                      # (no pad columns at this width: any raster position is a coefficient)
        n = v.size
        flat = np.zeros(n, dtype=np.int16)
        pos = [0, 5, 3100, 4095, 4096, 4096 + 3500, 8191, 8192, n - 1] if c == 0 else [1, 1023, 1024, 4097, 2048 + 4096, n - 2]
        for k, p in enumerate(p for p in pos if 0 <= p < n): flat[p] = vals[k % len(vals)]
        v[:] = flat.reshape(v.shape)
        if lv == 1:
            nz = np.flatnonzero(flat)
            for a, b in zip(nz[:-1], nz[1:]):
                # a run of 3072 zeros or more between two tokens of one segment of 4096 that crosses a window boundary
                if b - a - 1 >= 3072 and a // 4096 == b // 4096 and a // 1024 != b // 1024: found = True
    assert found
    check_level23_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META))


def test_level2_level3_lengths_qbist_frame():
    import cfhd_testlib as T
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libcfhd_ref.so")):
        pytest.skip("the Qbist generator lives in the reference build (oracle/_ref)")
    frames, pitch = T.qbist_frames(10, 1, W, H)
    plan = Plan(W, H)
    coeffs = oracle_forward_yuv422(plan, frames[0], pitch)
    _, stats = check_level23_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META))
    assert all(st[2] == 0 for st in stats.values())


def synth_rg48(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    px = np.zeros((h, w, 3), np.float64)
    for k in range(3):
        px[:, :, k] = (np.sin(x / (19.0 + 5 * k) + seed) * np.cos(y / (13.0 + 3 * k)) * 0.35 + 0.5) * 60000 + (x * y % 257) * 8.0 + rng.normal(0, 300, (h, w))
    return np.clip(px, 0, 65535).astype(np.uint16).reshape(-1).view(np.uint8).copy(), w * 6


def check_dense_level1(plan, coeffs, **kw):
    base, st = encode(plan, coeffs, **kw)
    assert st[8] == 1024 and st[1] == 0
    want = product_write_sample_host(plan, coeffs, 1, meta_global=META, input_format=kw.get("input_format", COLOR_FORMAT_YUYV), color_space=kw.get("color_space", 2),
                                     progressive=0 if kw.get("interlaced") else 1)
    assert differs(base, want) is None, differs(base, want)
    got, st = encode(plan, coeffs, l1_dense=4096, **kw)
    assert st[8] == 4096
    assert differs(got, base) is None, "dense level 1 at 4096: " + differs(got, base)
    got, st = encode(plan, coeffs, l1_dense=4096, l2=4096, l3=2048, **kw)
    assert differs(got, base) is None, "4096 / 4096 / 2048: " + differs(got, base)
    return st


@pytest.mark.parametrize("content", ["synthetic", "impulses", "qbist"])
def test_dense_level1_lengths_rg48(content):
    plan = Plan(RW, RH, pixkind=PIXKIND["RG48"], enc=ENC["444"])
    if content == "qbist":
        import cfhd_testlib as T
        if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libcfhd_ref.so")):
            pytest.skip("the Qbist generator lives in the reference build (oracle/_ref)")
        frames, pitch = T.qbist_frames(10, 1, RW, RH, PIX_RG48)
        frame = frames[0]
    else:
        frame, pitch = synth_rg48(RW, RH, 4)
    coeffs = oracle_forward_planes(plan, rg48_planes(frame, pitch, RW, RH))
    if content == "impulses":
        for c in range(3):
            for b in (1, 2, 3):
                d, v = plan.band[(c, 0, b)], plan.view(coeffs, c, 0, b)
                assert d["pitch"] == d["width"]
                flat = np.zeros(v.size, dtype=np.int16)
                for k, p in enumerate([0, 7, 3200, 4095, 4096, 4096 + 3600, 8191, 8192, v.size - 1]): flat[p] = [5000, -7000, 1023, -1024, 2, -1, 1500, -3000, 9][k]
                v[:] = flat.reshape(v.shape)
    check_dense_level1(plan, coeffs, input_format=COLOR_FORMAT_RG48, color_space=0)


def test_interlaced_plan_keeps_1024_in_table1_bands():
    """Interlaced frames: the difference-coded band (table 1, peaks) keeps segments of 1024 whatever the rule asks; the other level-1 bands, counted densely, and the bands
    of levels 2 and 3 take the long segments and give the same sample."""
    frame, pitch = synth_yuy2(W, H, 6)
    plan = Plan(W, H, progressive=0)
    from cfhd_testlib import oracle_forward_interlaced_yuv422
    coeffs = oracle_forward_interlaced_yuv422(plan, frame, pitch)
    base, st0 = encode(plan, coeffs, interlaced=1)
    want = product_write_sample_host(plan, coeffs, 1, meta_global=META, progressive=0)
    assert differs(base, want) is None, differs(base, want)
    for l1, l2, l3 in ((4096, 4096, 2048), (8192, 8192, 8192), (1024, 2048, 4096)):
        got, st = encode(plan, coeffs, l1_dense=l1, l2=l2, l3=l3, interlaced=1)
        assert st[4] > 0 and st[5] == 1024 and st[4] == st0[4]      # table-1 segments: as many, as long as before
        assert st[8] == l1 and st[1] > 0
        assert differs(got, base) is None, "l1=%d l2=%d l3=%d: %s" % (l1, l2, l3, differs(got, base))
