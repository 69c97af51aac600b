"""Grid size never changes what the chunk-indexed decoder computes, and the rule that picks the grids, on the CPU.

The kernels themselves (emu_entropy_decode_dx: k_dec_plan .. k_dec_tiles with `grid` workgroups for k_dec_index and k_dec_tiles, tiles of the product's size): the
coefficients of every coded band equal the oracle's pyramid, the harness expands the block lists through their masks and compares them with the dense bands (-50 / -51),
and the error word is clear (-10 - errors), for 1, 2, 7 and 10 workgroups -- 10 is what the emulated device's two compute units give k_dec_index alone.  One workgroup: every
wave strides over the chunks of a frame three times and more, and the prefetch one chunk / one tile ahead runs off the end; 7: no divisor of the work; 10: more workgroups
than tiles.  The emulated product: the same settings through GpuEntropyDecoder::launch_dx, whose clamps then apply.

The policy, from the emulator's launch trace (HIPEMU_TRACE, in a child process as tests/test_stream_batches_emulated.py does it): a pass queued beside an uncollected
one launches the shared grids, a pass queued alone the solo grids, a pass that failed no longer counts, the decode queue's passes count too, and
CFHD_AMD_DX_SHARED=0 turns the rule off."""
import ctypes, os, re, subprocess, sys
import numpy as np
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import hand_made_samples as S
    import dx_grid as D

    GRIDS = (1, 2, 7, 10)
    REPAIR_CASES = ("dense_small", "constant", "long_runs", "chunk_edges")


    def _emu_dx(sample, plan, mode, grid):
        E = emu()
        E.emu_entropy_decode_dx.argtypes = [c_u8p, ctypes.c_size_t, ctypes.c_int, c_i16p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
        got = np.full(plan.coeff_elems, 99, np.int16)
        s = np.frombuffer(sample, np.uint8).copy()
        return E.emu_entropy_decode_dx(p8(s), len(s), 1, p16(got), plan.coeff_elems, mode, grid), got


    def _check_kernels(sample, plan, modes, progressive, what):
        want = oracle_decode_pyramid(sample, plan)
        for mode in modes:
            for grid in GRIDS:
                rc, got = _emu_dx(sample, plan, mode, grid)
                assert rc == 0, "%s, mode %d, %d workgroups: %d" % (what, mode, grid, rc)
                for k in [k for k in plan.band if k[2] != 0]:
                    cols = plan.band[k]["width"] if not progressive else None
                    assert np.array_equal(plan.view(got, *k)[:, :cols], plan.view(want, *k)[:, :cols]), "%s, mode %d, %d workgroups: band %s" % (what, mode, grid, k)


    @pytest.mark.parametrize("name", S.NAMES)
    def test_hand_made_samples_on_the_kernels_under_every_grid(name):
        """Mode 8: host parser, speculation on; + 1 for the cases made for it: every chunk through the repair path."""
        c = S.case(name)
        _check_kernels(c.sample, c.plan, (8, 9) if name in REPAIR_CASES else (8,), c.progressive, name)


    @pytest.mark.parametrize("i", range(D.N))
    def test_batch_frames_on_the_kernels_under_every_grid(i):
        """Frame i of the 320 x 192 batch, its sample by the oracle's transform + the host writer (what the product writes: dx_grid.check_batch).  Mode 10: two copies in
        "device" memory, parsed by k_dec_parse and numbered by k_dec_plan / k_dec_plan_fill -- the frame queue's route --; 9: the repair path."""
        plan, coeffs = D.want_samples()
        sample = product_write_sample_host(plan, coeffs[i], i + 1, meta_global=S.META)
        # (a workgroup of k_dec_index is four waves: one workgroup strides three times and more over a frame of twelve chunks)
        assert len(sample) >= 12 * S.DX_CHUNK_BYTES, "frame %d: %d bytes are fewer than twelve chunks" % (i, len(sample))
        _check_kernels(sample, plan, (10, 9), 1, "frame %d" % i)


    @pytest.fixture(scope="module")
    def default_batch():
        with emulated_product():
            got = D.batch_round_trip(None)
            D.check_batch(got[0], got[1], "the library's own grids")
        return got


    @pytest.mark.parametrize("speculate", [True, False], ids=["speculating", "every-chunk-repaired"])
    @pytest.mark.parametrize("grid", [1, 2, 7])
    def test_emulated_batch_is_the_same_under_every_grid(default_batch, grid, speculate):
        with emulated_product():
            D.same_batches(D.batch_round_trip(grid, speculate), default_batch, "%d workgroups%s against the library's own grids" % (grid, "" if speculate else ", no speculation"))


    @pytest.mark.parametrize("name", ["mixed", "full_tile"])
    def test_emulated_hand_made_pictures_are_the_same_under_every_grid(name):
        with emulated_product():
            D.check_hand_made(name, (None, 1, 2, 7))


# ---- the policy ------------------------------------------------------------------------------------------------------------------------------------------------------
PW, PH = 336, 252        # one frame is some fifty chunks and more tiles than either tile grid: no clamp of launch_dx hides the shape


def _child():
    """Two frame-queue batches of one frame and a decode batch; every traced pass between marks on stderr."""
    import cfhd_testlib as T
    import dx_grid as D
    import decode_queue as DQ
    import hostile_pictures as HP
    with T.emulated_product():
        L = D.batch_api()
        good = T.synth_yuy2(PW, PH, 3)[0]
        a, b = (L.cfhd_amd_batch_create(PW, PH, T.PIX_YUY2, T.QUALITY_FILMSCAN1, 1, 1) for _ in range(2))
        assert a and b, T.amd_last_error()
        for x in (a, b): D.upload(L, x, 0, good, PW * 2)
        def mark(s): sys.stderr.write("[%s]\n" % s); sys.stderr.flush()
        def submit(x, name):
            mark(name + " begins"); rc = L.cfhd_amd_batch_submit(x); mark(name + " ends")
            assert rc == 0, T.amd_last_error()
        submit(a, "first alone"); submit(b, "second beside the first")
        assert L.cfhd_amd_batch_wait(a) > 0 and L.cfhd_amd_batch_wait(b) > 0, T.amd_last_error()
        submit(a, "alone again"); assert L.cfhd_amd_batch_wait(a) > 0
        # a pass that fails when it is collected (an oversize frame: -3) has left the count
        D.upload(L, b, 0, HP.yuy2("noise", PW, PH).reshape(-1), PW * 2)
        submit(b, "the failing pass")
        rc = L.cfhd_amd_batch_wait(b); assert rc == -3, rc
        submit(a, "behind the failed pass"); assert L.cfhd_amd_batch_wait(a) > 0
        # the synchronous entry point, beside nothing
        mark("synchronous begins"); assert L.cfhd_amd_batch_roundtrip(a) > 0; mark("synchronous ends")
        p = D.V(); n = ctypes.c_size_t()
        assert L.cfhd_amd_batch_get_sample(a, 0, ctypes.byref(p), ctypes.byref(n)) == 0
        sample = ctypes.string_at(p, n.value)
        # the decode queue: its pass counts for the frame queue's, and the frame queue's for it
        q = DQ.Queue(sample, "YUY2", DQ.FULL, 1)
        blob, offsets, sizes = DQ.pack([sample])
        mark("decode alone begins"); assert q.submit(blob, offsets, sizes) == 0, T.amd_last_error(); mark("decode alone ends")
        submit(a, "beside a decode pass")
        assert q.wait(1)[0] == 1 and L.cfhd_amd_batch_wait(a) > 0
        submit(a, "in front of a decode pass")
        mark("decode beside begins"); assert q.submit(blob, offsets, sizes) == 0, T.amd_last_error(); mark("decode beside ends")
        assert L.cfhd_amd_batch_wait(a) > 0 and q.wait(1)[0] == 1
        q.close(); L.cfhd_amd_batch_destroy(a); L.cfhd_amd_batch_destroy(b)


def _trace(shared):
    """{pass name: {kernel: grid.x}} of the persistent kernels of every marked pass."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    if not shared: env["CFHD_AMD_DX_SHARED"] = "0"
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    passes, name = {}, None
    for line in run.stderr.splitlines():
        m = re.match(r"\[(.+) begins\]$", line)
        if m: name = m.group(1); passes[name] = {}; continue
        if re.match(r"\[.+ ends\]$", line): name = None; continue
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
        if m and name:
            k = m.group(1).rsplit("::", 1)[-1]
            if k in ("k_dec_index", "k_dec_reindex", "k_dec_tiles"): passes[name][k] = int(m.group(3))
    return passes


# the emulated device has two compute units (tests/hipemu/hip/hip_runtime.h): 5 and 3 workgroups per unit alone, 2 and 2 beside other passes (cfhd_entropy_gpu.hip)
SOLO = {"k_dec_index": 10, "k_dec_reindex": 10, "k_dec_tiles": 6}
SHARED = {"k_dec_index": 4, "k_dec_reindex": 4, "k_dec_tiles": 4}
ALONE = ("first alone", "alone again", "behind the failed pass", "synchronous", "decode alone")
BESIDE = ("second beside the first", "beside a decode pass", "decode beside")


def test_a_pass_beside_another_launches_the_shared_grids():
    t = _trace(True)
    for name in ALONE: assert t[name] == SOLO, (name, t[name])
    for name in BESIDE: assert t[name] == SHARED, (name, t[name])


def test_the_policy_can_be_turned_off():
    t = _trace(False)
    for name in ALONE + BESIDE: assert t[name] == SOLO, (name, t[name])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child()
