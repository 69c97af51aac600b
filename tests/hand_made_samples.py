"""Hand-made samples for the chunk-indexed entropy decoder (tests/test_gpu_hand_made_samples.py on the hardware, tests/test_hand_made_samples.py pins them on the CPU):
code streams no encoder makes from a picture.  Each case builds a coefficient pyramid -- the oracle's forward transform of a flat mid-grey frame, so that the lowpass
bands keep the picture away from both clips, with chosen highpass bands overwritten (pad columns stay zero) -- and takes its sample from the host writer
(product_write_sample_host).  The C ABI decodes any sample, so the GPU suite reaches k_dec_index / k_dec_chain / k_dec_repair / k_dec_reindex / k_dec_tile_index /
k_dec_tiles with streams whose chunk, tile and piece boundaries are placed on purpose.

A plain module: the case table (`case(name)`), the writer's clamp and companding restated (`written_pyramid`), and the layout of a band's code words bit by bit
(`code_layout`), from which the builders steer payload sizes and the tests check where the runs lie.

Geometry 320 x 240: the luma level-1 bands hold 160 x 120 = 19 200 coefficients -- more than one LDS image of DX_TILE = 14 848, so two tiles, which dx_tile_plan makes
equal: 9728 each (`tile_len`) --, several 2016-byte chunks when dense; every band of levels 1 and 2 has pitch == width (flat raster positions are coefficient numbers), and
the band width is a multiple of 16 (the forced strip route with block lists is open).  `full_tile` alone uses 320 x 184: its luma level-1 bands (14 720 coefficients)
are one tile of the full 14 848, the only length at which k_dec_tiles stores the end of its image."""
import ctypes, functools
import numpy as np
from cfhd_testlib import *

W, H = 320, 240
META = b"GUID\x10\x00\x00G" + bytes(16)
DX_TILE, DX_CHUNK_BYTES = 14848, 2016          # cfhd_dec_kernels.h
LONG_RUN = 3072                                # zero runs from here on are past the run tables: copies of the longest composite code + a remainder
def tile_len(n):
    """Coefficients per tile of a band of n (cfhd_entropy_jobs.h dx_tile_plan): ceil(n / DX_TILE) tiles of equal length, a multiple of 512."""
    per = (n + DX_TILE - 1) // DX_TILE
    return ((n + per - 1) // per + 511) // 512 * 512


PROGRESSIVE = ("one_run", "corners", "dense_small", "long_words", "constant", "long_runs", "chunk_edges", "mixed")
EXTRA = ("full_tile",)                        # progressive too, of another geometry: not among the eight of the gathered launch
NAMES = PROGRESSIVE + EXTRA + ("interlaced_peaks",)
PEAK_THRESHOLD = 250                           # codec.h:155
LEVEL1 = [(c, 0, b) for c in range(3) for b in (1, 2, 3)]


class Case:
    """name, geometry, plan (8-bit 4:2:2 output), the quantized pyramid that was written, the sample, the bands that were overwritten by hand."""
    def __init__(self, name, w, h, coeffs, overwritten, progressive=1, **notes):
        self.name, self.w, self.h, self.progressive, self.overwritten, self.notes = name, w, h, progressive, list(overwritten), notes
        self.plan = Plan(w, h, progressive=progressive)
        self.coeffs = coeffs
        self.sample = product_write_sample_host(self.plan, coeffs, 1, meta_global=META, progressive=progressive)


def grey_pyramid(w, h, progressive=1):
    plan = Plan(w, h, progressive=progressive)
    frame = np.full(h * w * 2, 128, np.uint8)
    fwd = oracle_forward_yuv422 if progressive else oracle_forward_interlaced_yuv422
    return plan, fwd(plan, frame, w * 2)


def flat(plan, coeffs, key):
    """The band as a flat raster (a view); only for bands without pad columns."""
    d = plan.band[key]
    assert d["pitch"] == d["width"], key
    return plan.view(coeffs, *key).reshape(-1)


def small_values(rng, n, top=39):
    """Magnitude 1..top, random sign: code words of 2 to 12 bits with the sign."""
    return (rng.integers(1, top + 1, n) * rng.choice([-1, 1], n)).astype(np.int16)


# ---- the host writer's code, restated for the layout of a band ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def code_sizes(codebook=1):
    """(run_size[3072], run_count[3072], value_size[2048] by 11-bit two's complement value, band_end_size) of the host writer's tables."""
    rs = (ctypes.c_int * 3072)(); rc = (ctypes.c_int * 3072)(); vs = (ctypes.c_int * 2048)(); be = ctypes.c_int()
    hooks().cfhd_amd_code_sizes(codebook, rs, rc, vs, ctypes.byref(be))
    return np.array(rs), np.array(rc), np.array(vs), be.value


def run_bits(count, codebook=1):
    """Bits the writer's greedy loop spends on `count` zeros (vlc_encode_band put_run)."""
    rs, rc, _, _ = code_sizes(codebook)
    bits = 0
    while count > 0:
        idx = min(count, 3071)
        bits += int(rs[idx]); count -= int(rc[idx])
    return bits


def value_bits(v, codebook=1):
    _, _, vs, _ = code_sizes(codebook)
    v = np.clip(np.asarray(v, np.int64), -1023, 1023)
    return vs[np.where(v < 0, v + 2048, v)]


def code_layout(band, codebook=1):
    """Where the code words of a band lie in its payload.  band: the raster the writer walks (height x pitch flattened, pad columns zero -- the runs go through them).
    Returns (runs, payload_bytes): runs = [(first zero, zeros, first bit, bit behind the run's last code word)], the trailing run included; payload_bytes = the code words,
    the band end marker and the padding to a whole longword."""
    band = np.asarray(band).reshape(-1)
    nz = np.flatnonzero(band)
    vb = value_bits(band[nz], codebook)
    runs = []; bit = 0; at = 0
    for p, b in zip(nz.tolist(), vb.tolist()):
        if p > at:
            n = run_bits(p - at, codebook); runs.append((at, p - at, bit, bit + n)); bit += n
        bit += b; at = p + 1
    if at < band.size:
        n = run_bits(band.size - at, codebook); runs.append((at, band.size - at, bit, bit + n)); bit += n
    bit += code_sizes(codebook)[3]
    return runs, (bit + 31) // 32 * 4


def band_payloads(sample, nch=3):
    """{(c, lv, b): (offset, bytes, code set, peak level)} as the product's host parser finds the coded bands."""
    out = (ctypes.c_int * (nch * 9 * 4))()
    s = np.frombuffer(sample, np.uint8).copy()
    n = hooks().cfhd_amd_band_payloads(p8(s), ctypes.c_size_t(len(sample)), out)
    assert n == nch * 36, n
    keys = [(c, lv, b) for c in range(nch) for lv in range(3) for b in (1, 2, 3)]
    return {k: tuple(out[4 * i: 4 * i + 4]) for i, k in enumerate(keys)}


def written_pyramid(case):
    """What a decoder must make of case.coeffs, dequantized, lowpass raw: the writer clamps to +-1023 and codes the magnitude through the companding curve (code set 17:
    cubic, index + index^3 * 768 >> 24; test_host_bitstream.test_parse_and_host_decode_roundtrip), the decoder expands and multiplies by the band's divisor.  The
    difference-coded band of an interlaced sample (level 1, band 2: code set 18, linear) carries values beyond +-250 exactly in its peak table, and every row comes
    back as its running sum (finish_difference_band)."""
    plan = case.plan
    idx = np.arange(256)
    expand = idx + ((idx.astype(np.int64) ** 3 * 768) >> 24)
    inv = np.zeros(1025, np.int64); inv[np.minimum(expand[1:], 1023)] = idx[1:]; inv = np.maximum.accumulate(inv)
    out = np.zeros(plan.coeff_elems, np.int16)
    for (c, lv, b), d in plan.band.items():
        q = plan.view(case.coeffs, c, lv, b).astype(np.int64)
        if b == 0:
            if lv == 2: plan.view(out, c, lv, b)[:] = q
            continue
        if not case.progressive and (lv, b) == (0, 2):
            assert np.abs(q).max() * d["quant"] < 32768
            deq = np.cumsum(q[:, : d["width"]] * d["quant"], axis=1)
            assert np.abs(deq).max() < 32768, "a running sum leaves 16 bits"
            plan.view(out, c, lv, b)[:, : d["width"]] = deq
            continue
        plan.view(out, c, lv, b)[:] = np.sign(q) * expand[inv[np.minimum(np.abs(q), 1023)]] * d["quant"]
    return out


# ---- band builders ------------------------------------------------------------------------------------------------------------------------------------------------
def dense_band(n, seed):
    return small_values(np.random.default_rng(seed), n)


def long_runs_band(n, variant, seed):
    """Isolated values in a band of n coefficients, by flat raster position.
    variant 0: values on 511 and 512 (the boundary of the block lists' 64-block chunks); 3099 zeros behind them, inside the first payload chunk; a dense stretch whose
    length is searched so that the code words of the next run -- 3500 zeros -- straddle payload bit 2016 * 8; in bands of two tiles values on 14 847 and 14 848, the last
    coefficient of tile 0 and the first of tile 1; a value on the last coefficient.
    variant 1: the band starts with 3200 zeros; runs of 3999 zeros, one of them across coefficient 14 848; a value on the last coefficient."""
    rng = np.random.default_rng(seed)
    band = np.zeros(n, np.int16)
    band[n - 1] = -3
    if variant == 1:
        for k, p in enumerate(p for p in (3200, 8000, 12000, 16000) if p < n - 1): band[p] = (5, -2, 1, -9)[k]
        return band
    band[511] = 4; band[512] = -6; band[3612] = 2
    if DX_TILE < n - 1: band[DX_TILE - 1] = 7; band[DX_TILE] = -8
    if tile_len(n) < n - 1: band[tile_len(n) - 1] = -1; band[tile_len(n)] = 13
    first = 3613
    stretch = small_values(rng, 3600)
    for length in range(1200, 3600):                                           # (the stretch grows by one value at a time)
        trial = band.copy()
        trial[first: first + length] = stretch[:length]
        nxt = first + length + 3500
        if nxt >= n - 1: break
        trial[nxt] = 11
        runs, _ = code_layout(trial)
        r = next(r for r in runs if r[0] == first + length)
        if r[2] < DX_CHUNK_BYTES * 8 < r[3] and r[1] >= LONG_RUN: return trial
    raise AssertionError("no dense stretch puts the run across the chunk boundary")


def chunk_edge_band(n, want, seed):
    """A band of n coefficients, zero except for its last K: K is searched so that the payload (code words, end marker, padding) ends `want` of a 2016-byte chunk:
    "just_over": the last chunk holds 4 or 8 bytes; "full": the last chunk is full or within 8 bytes of full.  Two chunks at least."""
    vals = dense_band(n, seed)
    vb = value_bits(vals)
    end = code_sizes()[3]
    tail = np.concatenate([[0], np.cumsum(vb[::-1])])        # bits of the last K values
    for K in range(400, n):
        nbytes = (run_bits(n - K) + int(tail[K]) + end + 31) // 32 * 4
        rem = nbytes % DX_CHUNK_BYTES
        if nbytes > DX_CHUNK_BYTES and (0 < rem <= 8 if want == "just_over" else (rem == 0 or rem >= DX_CHUNK_BYTES - 8)):
            band = np.zeros(n, np.int16); band[n - K:] = vals[n - K:]
            return band, nbytes
    raise AssertionError("no count of values gives the payload size")


def _set_long_words(v, width):
    """Values up to the +-1023 clamp, scattered as tests/test_kernels_emulated.py does: code words of 13 to 26 bits, both escape levels of the long tables."""
    v[:] = 0
    a = v[:, :width]
    a[::7, ::5] = 1023; a[1::9, 2::11] = -1023; a[3::5, 1::13] = 300
    a[2::11, 3::7] = -150; a[5::13, ::9] = 64; a[4::17, 4::19] = 1500       # (1500: beyond the clamp, written as 1023)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------------
def _one_run():
    plan, co = grey_pyramid(W, H)
    for k in LEVEL1: plan.view(co, *k)[:] = 0
    return Case("one_run", W, H, co, LEVEL1)


def _corners():
    plan, co = grey_pyramid(W, H)
    for i, k in enumerate(LEVEL1):
        f = flat(plan, co, k); f[:] = 0; f[0] = (-5, 3, 9)[i % 3]; f[-1] = (7, -2, -12)[i % 3]
    return Case("corners", W, H, co, LEVEL1)


def _dense_small():
    plan, co = grey_pyramid(W, H)
    keys = [(0, 0, b) for b in (1, 2, 3)]
    for k in keys: flat(plan, co, k)[:] = dense_band(plan.band[k]["width"] * plan.band[k]["height"], 20 + k[2])
    return Case("dense_small", W, H, co, keys)


def _long_words():
    plan, co = grey_pyramid(W, H)
    keys = [(0, 0, 1), (0, 1, 2), (0, 2, 3)]           # one band of each level: k_dec_index's second- and third-level lookups, k_dec_tiles' trimmed path
    for k in keys: _set_long_words(plan.view(co, *k), plan.band[k]["width"])
    return Case("long_words", W, H, co, keys)


def _constant():
    """One value in every position: the same code word over and over, a bit pattern that parses at several alignments.  (The emulated twin in test_kernels_emulated.py
    uses 720 x 480; the conditions test_hand_made_samples.py sets -- alternates taken, chunks re-indexed, none repaired serially -- hold at 320 x 240 already.)"""
    plan, co = grey_pyramid(W, H)
    keys = [((0, 0, 2), 3), ((1, 0, 1), -7), ((0, 1, 2), 21)]
    for k, val in keys:
        v = plan.view(co, *k); v[:] = 0; v[:, : plan.band[k]["width"]] = val
    return Case("constant", W, H, co, [k for k, _ in keys])


def _long_runs():
    plan, co = grey_pyramid(W, H)
    keys = [(0, 0, 1), (0, 0, 2), (0, 0, 3)]
    for i, k in enumerate(keys): flat(plan, co, k)[:] = long_runs_band(19200, (0, 1, 0)[i], 30 + i)
    return Case("long_runs", W, H, co, keys)


def _chunk_edges():
    plan, co = grey_pyramid(W, H)
    flat(plan, co, (0, 0, 1))[:], a = chunk_edge_band(19200, "just_over", 41)
    flat(plan, co, (0, 0, 2))[:], b = chunk_edge_band(19200, "full", 42)
    return Case("chunk_edges", W, H, co, [(0, 0, 1), (0, 0, 2)], payload_bytes={(0, 0, 1): a, (0, 0, 2): b})


def _mixed():
    plan, co = grey_pyramid(W, H)
    for b in (1, 2, 3):
        flat(plan, co, (0, 0, b))[:] = dense_band(19200, 50 + b)                    # luma: dense_small
        plan.view(co, 1, 0, b)[:] = 0                                               # V: one_run
        flat(plan, co, (2, 0, b))[:] = long_runs_band(9600, (0, 1, 0)[b - 1], 60 + b)      # U: long_runs (one tile: 9600 coefficients)
    return Case("mixed", W, H, co, LEVEL1)


FULL_TILE_GEOMETRY = (320, 184)


def _full_tile():
    """Luma level-1 bands of 160 x 92 = 14 720 coefficients: one tile of the full DX_TILE, whose image a workgroup uses to its last word.  Band 1 ends in 1024 values,
    band 2 holds two values far from its end, band 3 is one run: a workgroup that decodes them one after the other (CFHD_AMD_DX_GRID_TILES=1) must have cleared the
    end of the image in between."""
    w, h = FULL_TILE_GEOMETRY
    plan, co = grey_pyramid(w, h)
    n = 14720
    assert tile_len(n) == DX_TILE and plan.band[(0, 0, 1)]["pitch"] * plan.band[(0, 0, 1)]["height"] == n
    f = flat(plan, co, (0, 0, 1)); f[:] = 0; f[n - 1024:] = dense_band(1024, 80)
    f = flat(plan, co, (0, 0, 2)); f[:] = 0; f[100] = 5; f[7000] = -4
    plan.view(co, 0, 0, 3)[:] = 0
    return Case("full_tile", w, h, co, [(0, 0, 1), (0, 0, 2), (0, 0, 3)])


def _interlaced_peaks():
    """Interlaced plan: level 1 is the field transform, its band 2 (subband 8) is coded in code set 18 as differences along the row, values beyond +-250 as +-251 with
    the true value in a peak table behind the band.  Hand-made: rows of small steps, rows with steps beyond the threshold (up to 1800: times the divisor still a 16-bit word of the peak table), row 0 and every eighth row left zero -- with the zero tail of the row in front, one long run."""
    plan, co = grey_pyramid(W, H, progressive=0)
    rng = np.random.default_rng(70)
    keys = [(c, 0, 2) for c in range(3)]
    for c, lv, b in keys:
        d = plan.band[(c, lv, b)]
        v = plan.view(co, c, lv, b); v[:] = 0
        wd = d["width"]
        for r in range(d["height"]):
            if r % 8 == 0: continue                                                  # a row that is one run
            row = np.zeros(wd, np.int64)
            if r % 8 in (1, 2, 5):
                x = np.sort(rng.choice(wd - 1, 6, replace=False))
                mag = np.repeat(rng.choice([251, 300, 700, 1000, 1800], 3), 2)       # differences: up, then down again by as much, so that the running sums stay inside 16 bits
                row[x] = mag * np.where(np.arange(6) % 2 == 0, 1, -1) * (1 if r % 2 else -1)
            else:
                x = rng.choice(wd, wd // 4, replace=False); row[x] = rng.integers(-6, 7, x.size)
            if r % 8 == 7: row[: wd // 2] = 0                                        # the row starts with a run
            v[r, :wd] = row
    return Case("interlaced_peaks", W, H, co, keys, progressive=0)


_BUILDERS = {"one_run": _one_run, "corners": _corners, "dense_small": _dense_small, "long_words": _long_words, "constant": _constant, "long_runs": _long_runs,
             "chunk_edges": _chunk_edges, "mixed": _mixed, "full_tile": _full_tile, "interlaced_peaks": _interlaced_peaks}


@functools.lru_cache(None)
def case(name):
    return _BUILDERS[name]()


# ---- what the tests compare with, computed once per case ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def want_yu64(name):
    """The oracle's YU64 picture of a progressive case (h x 2 w words): word-exact image of the decoded pyramid, no dither.  Read-only."""
    c = case(name)
    plan = Plan(c.w, c.h, pixkind=PIXKIND["YU64"])
    out = oracle_inverse_yu64(plan, oracle_decode_pyramid(c.sample, plan))[: c.h]
    out.flags.writeable = False
    return out


@functools.lru_cache(None)
def want_yuy2_interval(name):
    """(dither 0, dither 1) of the oracle's 8-bit 4:2:2 picture.  Read-only."""
    c = case(name)
    deq = oracle_decode_pyramid(c.sample, c.plan)
    inv = oracle_inverse_yuv422 if c.progressive else oracle_inverse_interlaced_yuv422
    lo, hi = inv(c.plan, deq, 0)[: c.h], inv(c.plan, deq, 1)[: c.h]
    lo.flags.writeable = False; hi.flags.writeable = False
    return lo, hi
