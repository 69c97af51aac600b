"""The hand-made samples of tests/hand_made_samples.py pinned on the CPU, so that a failure of tests/test_gpu_hand_made_samples.py means the hardware run differs and not
that a case is malformed: every case decodes, by the oracle and by the product's host parser, to the pyramid that was written; every case meets the conditions it was
made for (asserted, not reported); single-coefficient errors show in the YU64 picture the GPU tests compare; the bodies of the GPU tests pass on the emulated product;
where oracle/_ref is built, the reference decoder's YU64 picture equals the oracle's."""
import ctypes
import numpy as np
import pytest
from cfhd_testlib import *
import hand_made_samples as S
import test_gpu_hand_made_samples as G


def _coded_bands(plan):
    return [k for k in plan.band if k[2] != 0]


@pytest.mark.parametrize("name", S.NAMES)
def test_case_decodes_to_the_written_pyramid(name):
    """oracle_decode_pyramid == host_decode_pyramid == the pyramid that was written, values beyond the codebook's clamp held to the host writer's own clamp and
    companding (hand_made_samples.written_pyramid); the overwritten bands hold what the case says (pad columns zero)."""
    c = S.case(name)
    want = S.written_pyramid(c)
    got_o = oracle_decode_pyramid(c.sample, c.plan, lowpass_offset=0)
    got_h = host_decode_pyramid(c.sample, c.plan, lowpass_offset=0)
    for k in [k for k in c.plan.band if k[2] != 0 or k[1] == 2]:
        wd = c.plan.band[k]["width"]
        assert not c.plan.view(c.coeffs, *k)[:, wd:].any(), k
        assert np.array_equal(c.plan.view(got_o, *k)[:, :wd], c.plan.view(want, *k)[:, :wd]), ("oracle", k)
        assert np.array_equal(c.plan.view(got_h, *k)[:, :wd], c.plan.view(want, *k)[:, :wd]), ("host parser", k)
    assert c.overwritten and all(k in c.plan.band and k[2] != 0 for k in c.overwritten)


def _emu_dx(sample, plan, mode, grid):
    E = emu()
    E.emu_entropy_decode_dx.argtypes = [c_u8p, ctypes.c_size_t, ctypes.c_int, c_i16p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    E.emu_dx_stats.restype = ctypes.POINTER(ctypes.c_uint32)
    got = np.full(plan.coeff_elems, 99, np.int16)
    s = np.frombuffer(sample, np.uint8).copy()
    rc = E.emu_entropy_decode_dx(p8(s), len(s), 1, p16(got), plan.coeff_elems, mode, grid)
    return rc, got, E.emu_dx_stats()


@pytest.mark.parametrize("mode", [8, 9], ids=["speculating", "every-chunk-repaired"])
@pytest.mark.parametrize("name", S.NAMES)
def test_case_on_the_emulated_decoder_kernels(name, mode):
    """The kernels themselves (emu_entropy_decode_dx, tiles of the product's size; + 1: no run-in speculation) rebuild the oracle's pyramid of every case, the
    interlaced one with its peak table and running sums included, every coded band with its pitch padding."""
    c = S.case(name)
    want = oracle_decode_pyramid(c.sample, c.plan)
    rc, got, _ = _emu_dx(c.sample, c.plan, mode, 3)
    assert rc == 0
    for k in _coded_bands(c.plan):
        cols = c.plan.band[k]["width"] if not c.progressive else None
        assert np.array_equal(c.plan.view(got, *k)[:, :cols], c.plan.view(want, *k)[:, :cols]), k


def test_constant_has_no_unique_alignment():
    """The assertions of test_dx_decoder_emulated_code_without_unique_alignment: many rounds, alternates taken, chunks re-indexed, no band repaired serially."""
    c = S.case("constant")
    rc, _, st = _emu_dx(c.sample, c.plan, 0, 4)
    assert rc == 0
    assert st[2] >= 20, "the constant bands were expected to need many rounds (%d)" % st[2]
    assert (st[3] >> 16) > 0 and st[13] > 0 and st[12] == 0, "candidates %d, re-indexed %d, bands repaired serially %d" % (st[3] >> 16, st[13], st[12])


@pytest.mark.parametrize("name", ["dense_small", "mixed"])
def test_dense_bands_span_chunks_and_tiles(name):
    c = S.case(name)
    pay = S.band_payloads(c.sample)
    for b in (1, 2, 3):
        d = c.plan.band[(0, 0, b)]
        band = c.plan.view(c.coeffs, 0, 0, b)
        assert band.all() and np.abs(band).max() <= 39
        assert pay[(0, 0, b)][1] >= 2 * S.DX_CHUNK_BYTES + 1, "band %d: %d payload bytes are fewer than 3 chunks" % (b, pay[(0, 0, b)][1])
        assert d["pitch"] * d["height"] > S.DX_TILE, "one tile"
        assert S.code_layout(band)[1] == pay[(0, 0, b)][1]
    if name == "mixed":
        assert all(pay[(1, 0, b)][1] <= S.DX_CHUNK_BYTES for b in (1, 2, 3)), "the V bands were to hold one chunk each"
        assert max(pay[(0, 0, b)][1] for b in (1, 2, 3)) >= 10 * S.DX_CHUNK_BYTES


def test_one_run_and_corners_are_what_they_say():
    c = S.case("one_run")
    for k in S.LEVEL1:
        runs, nbytes = S.code_layout(c.plan.view(c.coeffs, *k))
        assert len(runs) == 1 and runs[0][:2] == (0, c.plan.band[k]["pitch"] * c.plan.band[k]["height"]) and nbytes == S.band_payloads(c.sample)[k][1]
    c = S.case("corners")
    for k in S.LEVEL1:
        f = c.plan.view(c.coeffs, *k).reshape(-1)
        assert f[0] and f[-1] and np.count_nonzero(f) == 2


def test_chunk_edges_payload_sizes():
    """One band whose last chunk holds at most 8 payload bytes, one whose last chunk is full or within 8 bytes of full -- by the host parser's byte counts."""
    c = S.case("chunk_edges")
    pay = S.band_payloads(c.sample)
    a, b = pay[(0, 0, 1)][1], pay[(0, 0, 2)][1]
    assert (a, b) == (c.notes["payload_bytes"][(0, 0, 1)], c.notes["payload_bytes"][(0, 0, 2)])
    assert a > S.DX_CHUNK_BYTES and 0 < a % S.DX_CHUNK_BYTES <= 8, a
    assert b > S.DX_CHUNK_BYTES and (b % S.DX_CHUNK_BYTES == 0 or b % S.DX_CHUNK_BYTES >= S.DX_CHUNK_BYTES - 8), b


def _inside_and_across(runs):
    """Of the zero runs of 3072 and more: how many have all their code words inside one 2016-byte chunk, how many have code words on both sides of a chunk boundary."""
    cb = S.DX_CHUNK_BYTES * 8
    long = [r for r in runs if r[1] >= S.LONG_RUN]
    return sum(1 for r in long if r[2] // cb == (r[3] - 1) // cb), sum(1 for r in long if r[2] // cb != (r[3] - 1) // cb)


def test_long_runs_lie_where_they_should():
    """From the layout of the code words (checked against the payload sizes the host parser reports): a run of 3072 or more inside one chunk, one across a chunk boundary,
    one across the boundary of the band's two tiles (9728) and one across coefficient 14 848; values on 511 / 512, 9727 / 9728, 14 847 / 14 848 and the last coefficient."""
    c = S.case("long_runs")
    pay = S.band_payloads(c.sample)
    inside = across = over_tile = over_image = 0
    for k in c.overwritten:
        band = c.plan.view(c.coeffs, *k).reshape(-1)
        runs, nbytes = S.code_layout(band)
        assert nbytes == pay[k][1], "the layout of band %s does not add up to the payload the parser found" % (k,)
        i, a = _inside_and_across(runs)
        inside += i; across += a
        over_tile += sum(1 for r in runs if r[0] < S.tile_len(band.size) < r[0] + r[1] and r[1] >= S.LONG_RUN)
        over_image += sum(1 for r in runs if r[0] < S.DX_TILE < r[0] + r[1] and r[1] >= S.LONG_RUN)
        assert band[-1]
    assert inside >= 1 and across >= 1 and over_tile >= 1 and over_image >= 1, (inside, across, over_tile, over_image)
    f = c.plan.view(c.coeffs, 0, 0, 1).reshape(-1)
    assert S.tile_len(f.size) == 9728
    assert all(f[p] for p in (511, 512, 9727, 9728, S.DX_TILE - 1, S.DX_TILE)) and not f[513:3612].any()
    u = S.case("mixed")
    i, a = 0, 0
    for b in (1, 2, 3):
        r = _inside_and_across(S.code_layout(u.plan.view(u.coeffs, 2, 0, b))[0]); i += r[0]; a += r[1]
    assert i >= 1 and a >= 1, "the U bands of `mixed`: %d runs inside a chunk, %d across" % (i, a)


def test_full_tile_fills_the_image():
    c = S.case("full_tile")
    for b in (1, 2, 3): assert S.tile_len(c.plan.band[(0, 0, b)]["pitch"] * c.plan.band[(0, 0, b)]["height"]) == S.DX_TILE
    f1, f2 = (c.plan.view(c.coeffs, 0, 0, b).reshape(-1) for b in (1, 2))
    assert f1[-1024:].all() and not f1[:-1024].any() and f2.any() and not f2[-2048:].any() and not c.plan.view(c.coeffs, 0, 0, 3).any()


def test_interlaced_peaks_carries_a_peak_table():
    c = S.case("interlaced_peaks")
    s = c.sample
    levels = [int.from_bytes(s[i + 2:i + 4], "big") for i in range(0, len(s) - 4, 4) if s[i:i + 2] == b"\xff\xb6"]      # TAG_PEAK_LEVEL (optional)
    assert any(levels), "no nonzero TAG_PEAK_LEVEL"
    pay = S.band_payloads(s)
    for ch in range(3):
        assert pay[(ch, 0, 2)][2:] == (2, S.PEAK_THRESHOLD * c.plan.band[(ch, 0, 2)]["quant"])
        v = c.plan.view(c.coeffs, ch, 0, 2)
        assert (np.abs(v) > S.PEAK_THRESHOLD).any() and not v[0].any() and not v[8].any()


@pytest.mark.parametrize("name", S.PROGRESSIVE + S.EXTRA)
def test_a_wrong_coefficient_shows_in_the_yu64_picture(name):
    """A clipped picture would hide a wrong coefficient.  200 coded highpass coefficients from a seeded generator, half of them from the overwritten bands, each
    perturbed alone by one divisor of its band in the oracle-decoded pyramid: at least 95 % change the oracle's YU64 picture."""
    c = S.case(name)
    plan = Plan(c.w, c.h, pixkind=PIXKIND["YU64"])
    deq = oracle_decode_pyramid(c.sample, plan)
    base = S.want_yu64(name)
    rng = np.random.default_rng(5)
    every = _coded_bands(plan)
    seen = 0
    for i in range(200):
        pool = c.overwritten if i % 2 == 0 else every
        k = pool[int(rng.integers(len(pool)))]
        d = plan.band[k]
        r, x = int(rng.integers(d["height"])), int(rng.integers(d["width"]))
        at = d["offset"] + r * d["pitch"] + x
        p = deq.copy()
        p[at] = p[at] + d["quant"] if p[at] + d["quant"] <= 32767 else p[at] - d["quant"]
        seen += not np.array_equal(oracle_inverse_yu64(plan, p)[: c.h], base)
    assert seen >= 190, "only %d of 200 single-coefficient errors change the YU64 picture of %s" % (seen, name)


# ---- the GPU tests' bodies on the emulated product (all eight handles in the gathered case) -------------------------------------------------------------------
def _gpu_bodies():
    out = []
    for name in ("full_tile", "mixed"):
        out += [pytest.param(G.test_yu64_when_a_workgroup_decodes_tile_after_tile, {"name": name, "grid": g}, id="test_yu64_when_a_workgroup_decodes_tile_after_tile[%s-%s]" % (name, g)) for g in ("1", "3")]
    for fn, axis, values in ((G.test_yu64_of_hand_made_samples_equals_oracle, "name", S.PROGRESSIVE + S.EXTRA), (G.test_yu64_of_hand_made_samples_without_speculation, "name", G.REPAIR_CASES),
                             (G.test_yuy2_of_hand_made_samples_block_lists_equal_dense_bands, "name", S.PROGRESSIVE + S.EXTRA),
                             (G.test_interlaced_peaks_sample_lies_in_the_oracle_interval, "route", ("default", "strip")), (G.test_gathered_launch_of_hand_made_samples, "out", ("YU64", "YUY2"))):
        out += [pytest.param(fn, {axis: v}, id="%s[%s]" % (fn.__name__, v)) for v in values]
    return out


@pytest.mark.parametrize("fn,kw", _gpu_bodies())
def test_on_the_emulated_product(fn, kw):
    with emulated_product():
        fn(**kw)


# ---- the reference decoder ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.ref
@pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")
@pytest.mark.parametrize("name", S.PROGRESSIVE + S.EXTRA)
def test_reference_decodes_the_case_to_the_oracles_yu64(name):
    c = S.case(name)
    want = S.want_yu64(name)
    def leg():
        dec, pitch = ref_decode_sample(c.sample, c.w, c.h, fourcc("YU64"))
        img = np.frombuffer(dec.tobytes(), np.uint16).reshape(c.h, pitch // 2)[:, : c.w * 2]
        return np.array_equal(img, want) or "%d words differ" % (img != want).sum()
    reference_leg(leg, 3, "hand-made 4:2:2 -> YU64")
