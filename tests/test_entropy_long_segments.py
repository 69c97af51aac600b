"""Level-1 segments longer than 1024 coefficients (cfhd_entropy_kernels.h ENT_SEG_L1, EntSegJob::len): the GPU entropy stage under the CPU emulation of
tests/hipemu writes the same sample, byte for byte, whatever the segment length of the level-1 bands (1024 .. 8192) and whichever kernel counts them (k_ent_count
over the dense bands, k_ent_count_blocks over block lists) -- and that sample is the product's host writer's."""
import ctypes, os
import numpy as np
import pytest
from cfhd_testlib import (ROOT, PRODUCT_DIR, Plan, _build_once, c_i16p, c_u8p, oracle_forward_yuv422, p8, p16, product_write_sample_host, synth_yuy2)

SO = os.path.join(ROOT, "tests", "_build", "libcfhd_emu_segments.so")
_lib = None
META = b"GUID\x10\x00\x00G" + bytes(range(16))


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(PRODUCT_DIR, "csrc"); hipemu = os.path.join(ROOT, "tests", "hipemu")
        src = os.path.join(hipemu, "emu_entropy_segments.cpp")
        host = [os.path.join(csrc, f) for f in ("cfhd_tables.cpp", "cfhd_bitstream.cpp", "cfhd_gop.cpp")]
        deps = [src, os.path.join(hipemu, "hip_emu.h"), os.path.join(hipemu, "cfhd_gfx950.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".cpp"))]
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        _build_once(SO, ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I" + hipemu, "-I" + csrc, src] + host, deps)
        L = ctypes.CDLL(SO)
        L.emu_entropy_encode_segments.restype = ctypes.c_long
        L.emu_entropy_encode_segments.argtypes = [ctypes.c_int] * 4 + [ctypes.c_uint, c_i16p, c_u8p, ctypes.c_size_t, c_u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_long)]
        _lib = L
    return _lib


def encode(plan, coeffs, l1_seg, count_mode, interlaced=0, frame_number=1):
    out = np.zeros(plan.width * plan.height * 8 + 65536, dtype=np.uint8)
    m = np.frombuffer(META, dtype=np.uint8).copy()
    stats = (ctypes.c_long * 5)()
    n = lib().emu_entropy_encode_segments(plan.width, plan.height, plan.pixkind, plan.quality, frame_number, p16(coeffs), p8(m), len(META), p8(out), out.size,
                                          interlaced, l1_seg, count_mode, stats)
    assert n > 0, n
    return bytes(out[:n]), list(stats)


def level1_views(plan, coeffs):
    for c in range(3):
        for b in (1, 2, 3):
            d = plan.band[(c, 0, b)]
            yield d, plan.view(coeffs, c, 0, b)


def check_all_lengths(plan, coeffs, want=None, lengths=(2048, 4096, 8192)):
    """The sample of 1024-coefficient segments (dense count: today's layout), equal to `want` when given, and every longer length through both count kernels."""
    base, st = encode(plan, coeffs, 1024, 0)
    assert st[1] == 0
    if want is not None:
        assert base == want
    for L in lengths:
        for mode in (0, 1):
            got, st = encode(plan, coeffs, L, mode)
            assert st[1] > 0                                    # (the level-1 bands did get long segments)
            if got != base:
                first = next(k for k in range(min(len(got), len(base))) if got[k] != base[k]) if len(got) == len(base) else -1
                raise AssertionError("L=%d count_mode=%d: %d bytes against %d, first difference at %d" % (L, mode, len(got), len(base), first))
    return base


@pytest.mark.parametrize("w,h,seed", [(336, 252, 3), (720, 480, 4)])
def test_long_segments_synthetic_frames(w, h, seed):
    frame, pitch = synth_yuy2(w, h, seed)
    plan = Plan(w, h)
    coeffs = oracle_forward_yuv422(plan, frame, pitch)
    check_all_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META))


def test_long_segments_qbist_frame():
    import cfhd_testlib as T
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libcfhd_ref.so")):
        pytest.skip("the Qbist generator lives in the reference build (oracle/_ref)")
    w, h = 640, 360
    frames, pitch = T.qbist_frames(10, 1, w, h)
    plan = Plan(w, h)
    coeffs = oracle_forward_yuv422(plan, frames[0], pitch)
    check_all_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META), lengths=(4096,))


def test_long_segments_noise_lists_every_block():
    """Every coefficient of the level-1 bands nonzero: every block listed, a segment of 4096 is four windows of tokens (the block kernel codes its token list
    between passes), and large values make segments wider than k_ent_emit's LDS window."""
    w, h = 320, 240
    plan = Plan(w, h)
    rng = np.random.default_rng(7)
    frame, pitch = synth_yuy2(w, h, 1)
    for amp in (3, 900):
        coeffs = oracle_forward_yuv422(plan, frame, pitch)
        for d, v in level1_views(plan, coeffs):
            v[:, : d["width"]] = rng.integers(1, amp + 1, size=(d["height"], d["width"])) * rng.choice([-1, 1], size=(d["height"], d["width"]))
        base = check_all_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META) if amp < 100 else None)      # (the host writer's buffer holds 4 bytes a pixel)
        _, st = encode(plan, coeffs, 4096, 1)
        if amp > 100:
            assert st[2] > 0 and st[3] > 32 * 1024        # segments beyond the LDS window: the payload takes the global atomics
        assert len(base) > 0


def test_long_segments_long_runs_and_large_values():
    """Isolated nonzeros: zero runs of 3072 and more inside one segment (past the run tables: the token takes k_ent_emit's table walk), runs that cross
    segments, values beyond +-1023 behind long runs, tokens on the first and last coefficient of segments and bands; bands end in the middle of a segment."""
    w, h = 640, 480
    plan = Plan(w, h)
    frame, pitch = synth_yuy2(w, h, 2)
    rng = np.random.default_rng(11)
    for variant in range(3):
        coeffs = oracle_forward_yuv422(plan, frame, pitch)
        for d, v in level1_views(plan, coeffs):
            flat = np.zeros(v.size, dtype=np.int16)
            n = flat.size
            pos = [0, 5, 3100, 4095, 4096, 4096 + 3500, 8191, 8192 + 7000, 3 * 8192 + 100, n - 1]
            if variant == 1: pos = [p + 1 for p in pos[:-1]] + [n - 2]
            if variant == 2: pos = sorted(set(int(x) for x in rng.integers(0, n, size=6)) | {n - 1})
            vals = [5000, -7000, 1023, -1024, 2, -1, 1500, -3000, 700, -2000, 4, 9]
            for k, p in enumerate(pos):
                if 0 <= p < n: flat[p] = vals[k % len(vals)]
            v[:] = flat.reshape(v.shape)
            v[:, d["width"]:] = 0                             # (pad columns stay zero: runs go through them)
        check_all_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META))


def test_long_segments_empty_level1_bands():
    """All-zero level-1 bands: segments without tokens, the band's whole payload is the trailing run."""
    w, h = 320, 240
    plan = Plan(w, h)
    frame, pitch = synth_yuy2(w, h, 5)
    coeffs = oracle_forward_yuv422(plan, frame, pitch)
    for d, v in level1_views(plan, coeffs): v[:] = 0
    check_all_lengths(plan, coeffs, want=product_write_sample_host(plan, coeffs, 1, meta_global=META))


def test_interlaced_encode_unchanged_by_long_segments():
    """Interlaced frames: the difference-coded band (table 1, peaks) keeps segments of 1024 whatever is asked; the table-0 level-1 bands, counted densely
    with long segments, give the same sample."""
    w, h = 336, 240
    plan = Plan(w, h)
    frame, pitch = synth_yuy2(w, h, 6)
    coeffs = oracle_forward_yuv422(plan, frame, pitch)
    base, st = encode(plan, coeffs, 1024, 0, interlaced=1)
    for L in (4096, 8192):
        got, st = encode(plan, coeffs, L, 0, interlaced=1)
        assert st[1] > 0 and got == base
