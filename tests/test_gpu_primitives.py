"""The primitives of cineform-sdk_amd/csrc/cfhd_gfx950.h on the hardware, one by one, against a numpy statement of each operation written here from the
comments of that header (NOT from the scalar twin tests/hipemu/cfhd_gfx950.h, which is a second implementation under test: tests/test_primitives_emulated.py runs
this whole file on the g++ build of the same translation unit, tests/gpu_prims/prims.hip, in the CPU suite).

Why: the kernels only ever reach these instructions with natural pictures, and the emulated suite replaces exactly this header.  Here every primitive sees the whole
int16 range, the saturation corners, wrap-around, every lane index and every store alignment."""
import ctypes
import numpy as np
import pytest
from cfhd_testlib import gfx950_prims

pytestmark = pytest.mark.gpu
EMULATED = False            # tests/test_primitives_emulated.py sets this around its calls

U32P = ctypes.POINTER(ctypes.c_uint32)
EXTREMES = np.array([-32768, -32767, -1, 0, 1, 32766, 32767], np.int64)


def _p(a): return a.ctypes.data_as(U32P)


def _call(name, *args):
    rc = getattr(gfx950_prims(EMULATED), "prim_" + name)(*args)
    assert rc == 0, "prim_%s -> %d" % (name, rc)


def pack(lo, hi): return ((lo.astype(np.int64) & 0xffff) | ((hi.astype(np.int64) & 0xffff) << 16)).astype(np.uint32)
def lanes(v):                                           # the two int16 lanes of packed words, as int64
    v = v.astype(np.int64)
    return ((v & 0xffff) ^ 0x8000) - 0x8000, ((v >> 16) ^ 0x8000) - 0x8000
def sat16(x): return np.clip(x, -32768, 32767)


def _pairs():
    """(a, b): all pairs from EXTREMES in both lanes (49 x 49 words), then 2^20 random pairs."""
    lo_a, lo_b, hi_a, hi_b = [g.reshape(-1) for g in np.meshgrid(EXTREMES, EXTREMES, EXTREMES, EXTREMES, indexing="ij")]
    rng = np.random.default_rng(5)
    r = rng.integers(0, 1 << 32, (2, 1 << 20), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([pack(lo_a, hi_a), r[0]]), np.concatenate([pack(lo_b, hi_b), r[1]])


# name -> the operation on int16 lanes (per lane: x, y -> int, wrapped to 16 bits by pack); from the header's comments:
#   pk_adds / pk_subs: "exactly SSE2's _mm_adds_epi16 / _mm_subs_epi16 on two lanes"; pk_addw / pk_negw / pk_maxs: "wrapping (non-saturating) packed add / negate and
#   signed max"; pk_mulw: "wrapping packed multiply, low halves of the products"
LANE_OPS = {
    "pk_adds": lambda x, y: sat16(x + y), "pk_subs": lambda x, y: sat16(x - y), "pk_addw": lambda x, y: x + y, "pk_maxs": lambda x, y: np.maximum(x, y),
    "pk_mulw": lambda x, y: (x & 0xffff) * (y & 0xffff),
}


@pytest.mark.parametrize("name", sorted(LANE_OPS))
def test_packed_arithmetic(name):
    a, b = _pairs()
    out = np.zeros_like(a)
    _call(name, _p(a), _p(b), _p(out), a.size)
    (al, ah), (bl, bh) = lanes(a), lanes(b)
    want = pack(LANE_OPS[name](al, bl), LANE_OPS[name](ah, bh))
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, "%s: %d of %d words differ, first a=%08x b=%08x got %08x want %08x" % (name, bad.size, a.size, a[bad[0]], b[bad[0]], out[bad[0]], want[bad[0]])


def test_pk_negw_sra_lolo_hihi():
    a, b = _pairs()
    al, ah = lanes(a)
    out = np.zeros_like(a)
    _call("pk_negw", _p(a), _p(out), a.size)
    assert np.array_equal(out, pack(-al, -ah))                                      # wrapping: -(-32768) = -32768
    for n in range(16):
        _call("pk_sra", _p(a), n, _p(out), a.size)
        assert np.array_equal(out, pack(al >> n, ah >> n)), "pk_sra by %d" % n      # arithmetic shift of each lane
    _call("pk_lolo", _p(a), _p(b), _p(out), a.size)
    assert np.array_equal(out, (a & 0xffff) | (b << 16))                            # (a.lo, b.lo)
    _call("pk_hihi", _p(a), _p(b), _p(out), a.size)
    assert np.array_equal(out, (a >> 16) | (b & 0xffff0000))                        # (a.hi, b.hi)


def to8(v, shift, d):
    """'10 -> 8 bits: clamp at zero, halve, add the dither bit, >> shift, saturate' (to 255), one lane."""
    return np.minimum(((np.maximum(v, 0) >> 1) + d) >> shift, 255)


def _all_int16_twice():
    """Every 16-bit value in the low lane and -- in another order -- in the high lane: two such words (e, o)."""
    x = np.arange(65536, dtype=np.int64)
    rot = lambda v, k: ((v << k) | (v >> (16 - k))) & 0xffff
    return pack(x, rot(x, 7)), pack(65535 - x, rot(x, 3) ^ 0x5a5a)


@pytest.mark.parametrize("shift1", range(1, 8))
def test_pk_to8_and_pk_to8_bytes_over_the_whole_int16_range(shift1):
    """Exhaustive: all 65 536 values in both lanes, dither bit 0 and 1 in each lane; pk_to8 against the statement above, pk_to8_bytes against 'equal to pk_to8 on both
    words, bytes in sample order' (e = (s0, s2), o = (s1, s3); d2e / d2o = twice the dither bit of each lane: bit 1, bit 17; shift1 = shift + 1), and the two against
    each other on the device's own outputs."""
    e1, o1 = _all_int16_twice()
    combos = np.arange(16)
    e = np.tile(e1, 16); o = np.tile(o1, 16)
    k = np.repeat(combos, 65536)
    de_lo, de_hi, do_lo, do_hi = k & 1, (k >> 1) & 1, (k >> 2) & 1, (k >> 3) & 1
    de = (de_lo | (de_hi << 16)).astype(np.uint32); do = (do_lo | (do_hi << 16)).astype(np.uint32)
    shift = shift1 - 1
    te = np.zeros_like(e); to = np.zeros_like(e); tb = np.zeros_like(e)
    _call("pk_to8", _p(e), shift, _p(de), _p(te), e.size)
    _call("pk_to8", _p(o), shift, _p(do), _p(to), e.size)
    d2e = (de << 1).astype(np.uint32); d2o = (do << 1).astype(np.uint32)
    _call("pk_to8_bytes", _p(e), _p(o), shift1, _p(d2e), _p(d2o), _p(tb), e.size)
    (el, eh), (ol, oh) = lanes(e), lanes(o)
    s0, s2, s1, s3 = to8(el, shift, de_lo), to8(eh, shift, de_hi), to8(ol, shift, do_lo), to8(oh, shift, do_hi)
    assert np.array_equal(te, pack(s0, s2)), "pk_to8: %d words differ" % (te != pack(s0, s2)).sum()
    assert np.array_equal(to, pack(s1, s3)), "pk_to8: %d words differ" % (to != pack(s1, s3)).sum()
    want = (s0 | (s1 << 8) | (s2 << 16) | (s3 << 24)).astype(np.uint32)
    bad = np.flatnonzero(tb != want)
    assert bad.size == 0, "pk_to8_bytes: %d of %d words differ, first e=%08x o=%08x d2e=%05x d2o=%05x got %08x want %08x" % (
        bad.size, e.size, e[bad[0]], o[bad[0]], d2e[bad[0]], d2o[bad[0]], tb[bad[0]], want[bad[0]])
    both = ((te & 0xff) | ((to & 0xff) << 8) | ((te >> 16) << 16) | ((to >> 16) << 24)).astype(np.uint32)
    assert np.array_equal(tb, both), "pk_to8_bytes and pk_to8 disagree on %d words" % (tb != both).sum()


# every selector constant of cineform-sdk_amd/csrc (grep byte_perm / __builtin_amdgcn_perm): the interleaves of the strip kernels' output, pk_lolo / pk_hihi / pk_to8_bytes,
# and usel / vsel of the forward strips = byte b of a0, zero, byte b of a1, zero for b = 0..3 (cfhd_kernels.h: b | 0x0c00 | (4 + b) << 16 | 0x0c000000)
SELECTORS = [0x05010400, 0x07030602, 0x01050004, 0x03070206, 0x05040100, 0x07060302] + [b | 0x0c00 | ((4 + b) << 16) | 0x0c000000 for b in range(4)]


@pytest.mark.parametrize("sel", SELECTORS, ids=["%08x" % s for s in SELECTORS])
def test_byte_perm_selectors(sel):
    """v_perm_b32: result byte k = byte sel[k] of the eight bytes (s0 : s1) -- 0..3 from s1, 4..7 from s0 --, selector 0x0c = the constant 0."""
    rng = np.random.default_rng(sel)
    s0, s1 = rng.integers(0, 1 << 32, (2, 4096), dtype=np.uint64).astype(np.uint32)
    out = np.zeros_like(s0)
    _call("byte_perm", _p(s0), _p(s1), _p(np.full_like(s0, sel)), _p(out), s0.size)
    src = (s0.astype(np.uint64) << 32) | s1
    want = np.zeros(s0.size, np.uint64)
    for k in range(4):
        b = (sel >> (8 * k)) & 0xff
        assert b < 8 or b == 0x0c
        if b < 8: want |= ((src >> np.uint64(8 * b)) & np.uint64(0xff)) << np.uint64(8 * k)
    assert np.array_equal(out, want.astype(np.uint32))


def test_rotr32_and_mul_u24():
    rng = np.random.default_rng(9)
    w = np.repeat(rng.integers(0, 1 << 32, 512, dtype=np.uint64), 32); n = np.tile(np.arange(32, dtype=np.uint64), 512)
    out = np.zeros(w.size, np.uint32)
    _call("rotr32", _p(w.astype(np.uint32)), _p(n.astype(np.uint32)), _p(out), w.size)
    assert np.array_equal(out, (((w >> n) | (w << (np.uint64(32) - n))) & np.uint64(0xffffffff)).astype(np.uint32))          # n in 0..31
    # mul_u24: "the low 16 bits equal those of the full product" -- whatever bits 24..31 of the operands hold
    a, b = rng.integers(0, 1 << 32, (2, 1 << 16), dtype=np.uint64)
    a[:256] |= 0xff000000; b[:256] |= 0xff000000
    out = np.zeros(a.size, np.uint32)
    _call("mul_u24", _p(a.astype(np.uint32)), _p(b.astype(np.uint32)), _p(out), a.size)
    assert np.array_equal(out & 0xffff, ((a * b) & np.uint64(0xffff)).astype(np.uint32))


def test_wave_scan_mbcnt_get_read():
    """Whole 64-lane waves, four to a workgroup, several workgroups: wave_incl_scan = inclusive prefix sum over the lanes of each wave (32-bit wrap-around);
    wave_mbcnt(ballot) = lanes below this one whose bit is set; wave_get / wave_read = the value of lane l of this wave, for every l."""
    rng = np.random.default_rng(11)
    waves = [np.zeros(64), np.ones(64), np.full(64, 0xffffffff), np.full(64, 0x80000000)] + [rng.integers(0, 1 << 32, 64, dtype=np.uint64) for _ in range(8)]
    x = np.concatenate(waves).astype(np.uint32)                                        # 12 waves = 3 workgroups
    preds = [np.zeros(64), np.ones(64)] + [rng.integers(0, 2, 64) for _ in range(10)]
    pred = np.concatenate(preds).astype(np.uint32)
    scan = np.zeros_like(x); mb = np.zeros_like(x)
    _call("wave_scan_mbcnt", _p(x), _p(pred), _p(scan), _p(mb), x.size)
    assert np.array_equal(scan.reshape(-1, 64), (np.cumsum(x.reshape(-1, 64).astype(np.uint64), axis=1) & np.uint64(0xffffffff)).astype(np.uint32))
    p = pred.reshape(-1, 64).astype(np.int64)
    assert np.array_equal(mb.reshape(-1, 64), np.cumsum(p, axis=1) - p)
    order = rng.permutation(64).astype(np.int32)
    get = np.zeros((64, x.size), np.uint32); read = np.zeros((64, x.size), np.uint32)
    _call("wave_get_read", _p(x), order.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _p(get), _p(read), x.size)
    xw = x.reshape(-1, 64)
    for l in range(64):
        assert np.array_equal(get[l].reshape(-1, 64), np.repeat(xw[:, l:l + 1], 64, axis=1)), "wave_get lane %d" % l
        assert np.array_equal(read[l].reshape(-1, 64), np.repeat(xw[:, order[l]:order[l] + 1], 64, axis=1)), "wave_read lane %d" % order[l]


@pytest.mark.parametrize("kind", [2, 4])
def test_vector_stores_at_every_dword_offset(kind):
    """store_u32x2_dword_aligned / store_u32x4_global at dword offsets 0..7 from a 32-byte aligned address: the words land, every other word -- the guard words on
    either side first of all -- keeps its pattern.  For store_u32x4_global only offsets 0 and 4 are inside its contract (a 16-byte aligned vector type); the others
    are driven here because gfx950 serves unaligned vector stores to global memory and the test then also shows that such a store touches its sixteen bytes and nothing
    else -- they are not supported use of the function."""
    for off in range(8):
        buf = (np.arange(32, dtype=np.uint32) * 0x01010101) ^ 0xdeadbeef
        before = buf.copy()
        vals = [0x11111111 * (k + 1) + off for k in range(4)]
        _call("store", _p(buf), buf.size, 8 + off, kind, *[ctypes.c_uint32(v) for v in vals])
        want = before.copy(); want[8 + off: 8 + off + kind] = vals[:kind]
        assert np.array_equal(buf, want), "offset %d: %s" % (off, np.flatnonzero(buf != want))


def test_global_loads_round_trip():
    pattern = (np.arange(4096, dtype=np.uint64) * 2654435761 & 0xffffffff).astype(np.uint32)
    for name in ("ldg32", "ldg64", "ldg128"):
        out = np.zeros_like(pattern)
        _call(name, _p(pattern), _p(out), pattern.size)
        assert np.array_equal(out, pattern), name
