"""Dense samples (cfhd_entropy_kernels.h k_ent_sizes, k_ent_pack_offsets, EntFrameJob::dense_off): a batch of frames of very different sizes through the GPU entropy
stage under the CPU emulation of tests/hipemu.  Every sample's size is known behind k_ent_scan, its 64-byte aligned place in ONE buffer follows from the sizes in front
of it, and k_ent_layout / k_ent_emit write it there: sizes, offsets and bytes must be the host writer's (write_sample(), through product_write_sample_host), the gaps
between samples and everything behind the last one untouched."""
import ctypes, os, subprocess
import numpy as np
import pytest
import cfhd_testlib as T
from cfhd_testlib import ROOT, PRODUCT_DIR, Plan, _build_once, c_i16p, c_u8p, oracle_forward_yuv422, p8, p16, product_write_sample_host

SO = os.path.join(ROOT, "tests", "_build", "libcfhd_emu_dense.so")
ASAN_EXE = os.path.join(ROOT, "tests", "_build", "dense_samples_asan")
META = b"GUID\x10\x00\x00G" + bytes(range(16))
GUARD = 0xA5
GEOMETRIES = [(256, 144), (176, 96)]      # width % 32 == 0: level-1 bands from block lists, segments of ENT_SEG_L1; width % 32 == 16: counted densely
_lib = None
_u32p = ctypes.POINTER(ctypes.c_uint32)


def _sources():
    csrc = os.path.join(PRODUCT_DIR, "csrc"); hipemu = os.path.join(ROOT, "tests", "hipemu")
    host = [os.path.join(csrc, f) for f in ("cfhd_tables.cpp", "cfhd_bitstream.cpp", "cfhd_gop.cpp")]
    deps = [os.path.join(hipemu, f) for f in ("emu_dense_samples.cpp", "dense_samples_asan_main.cpp", "hip_emu.h", "cfhd_gfx950.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".cpp"))]
    return csrc, hipemu, host, deps


def lib():
    global _lib
    if _lib is None:
        csrc, hipemu, host, deps = _sources()
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        _build_once(SO, ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I" + hipemu, "-I" + csrc, os.path.join(hipemu, "emu_dense_samples.cpp")] + host, deps)
        L = ctypes.CDLL(SO)
        L.emu_dense_encode.restype = ctypes.c_long
        L.emu_dense_encode.argtypes = [ctypes.c_int] * 5 + [c_i16p, c_u8p, ctypes.c_size_t, c_u8p, ctypes.c_size_t, ctypes.c_uint, _u32p, _u32p, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_long)]
        _lib = L
    return _lib


def five_frames(w, h):
    """Black, flat grey, a Qbist picture, uniform noise, the Qbist picture again (YUY2)."""
    pitch = w * 2
    black = np.zeros(h * pitch, dtype=np.uint8); black[0::2] = 16; black[1::2] = 128
    grey = np.full(h * pitch, 128, dtype=np.uint8)
    if T.have_ref():
        frames, qp = T.qbist_frames(10, 1, w, h)
        assert qp == pitch
        qbist = frames[0]
    else:
        qbist, qp = T.synth_yuy2(w, h, 10)                # (the Qbist generator lives in the reference build; without it: the suite's synthetic picture)
        assert qp == pitch
    noise = np.random.default_rng(w * 1000 + h).integers(0, 256, size=h * pitch, dtype=np.uint8)
    return [black, grey, qbist, noise, qbist], pitch


_cache = {}


def batch(w, h):
    """(plan, the five pyramids in one array, the host writer's five samples): computed once per geometry, never modified."""
    if (w, h) not in _cache:
        plan = Plan(w, h)
        frames, pitch = five_frames(w, h)
        pyr = [oracle_forward_yuv422(plan, f, pitch) for f in frames]
        want = [product_write_sample_host(plan, c, i + 1, meta_global=META) for i, c in enumerate(pyr)]
        coeffs = np.concatenate(pyr); coeffs.flags.writeable = False
        _cache[(w, h)] = (plan, coeffs, want)
    return _cache[(w, h)]


def encode(plan, coeffs, n, cap, parts=3, interlaced=0):
    """-> (sizes, offsets[n + 1], the dense buffer with its guard bytes, stats)."""
    room = ((cap + 63) & ~63) * n
    raw = np.full(room + 64 + 4096, GUARD, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 64
    packed = raw[skip: skip + room + 4096]
    sizes = np.full(n, 0xdeadbeef, dtype=np.uint32); offsets = np.full(n + 1, 0xdeadbeef, dtype=np.uint32)
    m = np.frombuffer(META, dtype=np.uint8).copy()
    stats = (ctypes.c_long * 3)()
    c = np.array(coeffs)                                  # (the count kernels take a writable pointer)
    rc = lib().emu_dense_encode(plan.width, plan.height, plan.pixkind, plan.quality, n, p16(c), p8(m), len(META), p8(packed), room, cap,
                                sizes.ctypes.data_as(_u32p), offsets.ctypes.data_as(_u32p), interlaced, parts, stats)
    assert rc == 0, rc
    assert (c == coeffs).all()
    return sizes, offsets, packed, list(stats)


def check_dense(sizes, offsets, packed, want):
    """want[i]: the sample's bytes, or None for a frame that must report size 0 and take no room."""
    at = 0
    for i, s in enumerate(want):
        assert offsets[i] == at and at % 64 == 0, (i, offsets[i], at)
        n = 0 if s is None else len(s)
        assert sizes[i] == n, (i, sizes[i], n)
        got = bytes(packed[at: at + n])
        if got != (s or b""):
            first = next(k for k in range(n) if got[k] != s[k])
            raise AssertionError("sample %d: first difference at byte %d of %d" % (i, first, n))
        nxt = at + ((n + 63) & ~63)
        assert (packed[at + n: nxt] == GUARD).all(), "sample %d: bytes written behind its end" % i
        at = nxt
    assert offsets[len(want)] == at
    assert (packed[at:] == GUARD).all(), "bytes written behind the last sample"


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_dense_batch_equals_host_writer(w, h):
    plan, coeffs, want = batch(w, h)
    cap = (w * h * 2 + 65536 + 255) & ~255                # the slot size of the batched encoder
    sizes, offsets, packed, st = encode(plan, coeffs, 5, cap)
    assert st[2] == (1 if w % 32 == 0 else 0)
    if w % 32 == 0: assert st[1] > 0                      # the noise frame's long level-1 segments do not fit k_ent_emit's LDS window: the wide-segment path writes into the dense buffer too
    assert len(want[3]) > 4 * len(want[0])               # noise against black: the offsets cannot be a stride
    check_dense(sizes, offsets, packed, want)


@pytest.mark.parametrize("w,h", GEOMETRIES)
@pytest.mark.parametrize("parts", [1, 8])
def test_dense_batch_other_layout_grids(w, h, parts):
    """k_ent_layout with one workgroup per frame and with more workgroups than some holes have pieces."""
    plan, coeffs, want = batch(w, h)
    sizes, offsets, packed, _ = encode(plan, coeffs, 5, (w * h * 2 + 65536 + 255) & ~255, parts=parts)
    check_dense(sizes, offsets, packed, want)


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_oversize_frame_takes_no_room(w, h):
    """A capacity below the noise frame's size and above every other: that frame reports size 0, takes no room, nothing of it is written, its neighbours are intact."""
    plan, coeffs, want = batch(w, h)
    others = max(len(s) for i, s in enumerate(want) if i != 3)
    assert others + 64 < len(want[3])
    cap = (others + 255) & ~255
    assert cap < len(want[3])
    sizes, offsets, packed, _ = encode(plan, coeffs, 5, cap)
    check_dense(sizes, offsets, packed, [s if i != 3 else None for i, s in enumerate(want)])
    assert offsets[4] == offsets[3]


def test_capacity_is_inclusive():
    """out_cap equal to the largest sample's size: every frame is written."""
    w, h = GEOMETRIES[1]
    plan, coeffs, want = batch(w, h)
    sizes, offsets, packed, _ = encode(plan, coeffs, 5, max(len(s) for s in want))
    check_dense(sizes, offsets, packed, want)


def peak_levels(sample):
    """TAG_PEAK_LEVEL of every band that has the three optional tags of a band coded with peaks (zero: no table)."""
    return [int.from_bytes(sample[i + 10:i + 12], "big") for i in range(0, len(sample) - 12, 4)
            if sample[i:i + 2] == b"\xff\xb5" and sample[i + 4:i + 6] == b"\xff\xb4" and sample[i + 8:i + 10] == b"\xff\xb6"]


def interlaced_batch(w, h):
    """Five interlaced frames: black, grey, Qbist, the field-flicker picture (its difference-coded bands carry peak tables), Qbist again."""
    plan = Plan(w, h, progressive=0)
    frames, pitch = five_frames(w, h)
    frames[3], fp = T.field_flicker_frame(w, h)
    assert fp == pitch
    pyr = [T.oracle_forward_interlaced_yuv422(plan, f, pitch) for f in frames]
    want = [product_write_sample_host(plan, c, i + 1, meta_global=META, progressive=0) for i, c in enumerate(pyr)]
    return plan, np.concatenate(pyr), want


def test_dense_batch_interlaced_peak_tables():
    """Interlaced plans: peak tables are written by k_ent_peaks through EntBandState::peak_out -- an address inside the dense buffer, behind samples without tables."""
    w, h = 176, 96
    plan, coeffs, want = interlaced_batch(w, h)
    assert any(peak_levels(want[3])) and not any(peak_levels(want[0]))
    sizes, offsets, packed, _ = encode(plan, coeffs, 5, (w * h * 2 + 65536 + 255) & ~255, interlaced=1)
    check_dense(sizes, offsets, packed, want)


def test_dense_samples_under_sanitizers():
    """The same batch driver as a stand-alone program built with -fsanitize=address,undefined: every buffer is exactly as large as the driver's arithmetic says (the
    dense buffer cap-rounded-to-64 x frames, offsets n + 1 words), so a store outside a sample's place or an offset sum that wraps is a report."""
    csrc, hipemu, host, deps = _sources()
    os.makedirs(os.path.dirname(ASAN_EXE), exist_ok=True)
    _build_once(ASAN_EXE, ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17", "-pthread",
                           "-I" + hipemu, "-I" + csrc, os.path.join(hipemu, "dense_samples_asan_main.cpp"), os.path.join(hipemu, "emu_dense_samples.cpp")] + host, deps)
    r = subprocess.run([ASAN_EXE], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1"))
    assert r.returncode == 0 and "dense samples ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
