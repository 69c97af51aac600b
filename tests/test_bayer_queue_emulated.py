"""tests/test_gpu_bayer_queue.py on the CPU against the emulated product library (cfhd_testlib.emulated_product), and what only the emulator can show: the launch
trace of a Bayer pass (HIPEMU_TRACE, in a child process) -- under CFHD_AMD_INVERSE=strip k_inv_bayer_strip once and neither kernel of the pair, under tile the pair
once each; the same kernels for 2 samples and for 8, only the grids grow; an intact pass launches nothing inside wait."""
import json, os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import bayer_queue as BQ


    @pytest.mark.parametrize("source", BQ.SOURCES)
    @pytest.mark.parametrize("w,h", BQ.SHAPES)
    def test_emulated_fused_last_level_equals_the_pair_equals_the_handle(w, h, source):
        if source == "ref" and not have_ref(): pytest.skip("oracle/_ref/libcfhd_ref.so is not built")
        with emulated_product():
            BQ.check_fused_equals_pair_equals_handle(w, h, source)


    @pytest.mark.parametrize("w,h", BQ.SHAPES)
    def test_emulated_a_short_pass_is_delivered_into_device_memory_and_nothing_else_is_touched(w, h):
        with emulated_product():
            BQ.check_short_pass_and_delivery(w, h)


    @pytest.mark.parametrize("w,h", BQ.SHAPES)
    def test_emulated_verdict_per_sample_under_both_routes(w, h):
        with emulated_product():
            BQ.check_verdicts(w, h)


    def test_emulated_gates():
        with emulated_product():
            BQ.check_gates()


    @pytest.mark.parametrize("w,h", BQ.SHAPES)
    def test_emulated_frame_queue_round_trip(w, h):
        with emulated_product():
            BQ.check_frame_queue_round_trip(w, h)


def _child(nsamples, mode):
    """One Bayer decode batch of 192 x 96 samples and one pass under CFHD_AMD_INVERSE=mode; the trace of the pass -- submit to wait -- to stderr."""
    import cfhd_testlib as T
    import decode_queue as DQ
    import bayer_queue as BQ
    with T.emulated_product():
        eight = BQ.samples_of(192, 96, "amd")
        samples = [eight[i % 8] for i in range(nsamples)]
        q = BQ.Queue(eight[0], nsamples)
        blob, offsets, sizes = DQ.pack(samples)
        os.environ["CFHD_AMD_INVERSE"] = mode
        sys.stderr.write("[pass begins]\n"); sys.stderr.flush()
        assert q.submit(blob, offsets, sizes) == 0, T.amd_last_error()
        sys.stderr.write("[submitted]\n"); sys.stderr.flush()
        ret, status = q.wait(nsamples)
        sys.stderr.write("[pass ends]\n"); sys.stderr.flush()
        name = q.last_level().decode()
        q.close()
    print("STATUS " + json.dumps([ret, status, name]))


def _trace(nsamples, mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(nsamples), mode], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ret, status, name = json.loads(next(line for line in run.stdout.splitlines() if line.startswith("STATUS "))[7:])
    lines = run.stderr.splitlines()
    def launches(a, b):
        out = []
        for line in lines[lines.index(a) + 1: lines.index(b)]:
            m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
            if m: out.append((m.group(1).rsplit("::", 1)[-1], tuple(int(m.group(k)) for k in (3, 4, 5))))
        return out
    return ret, status, name, launches("[pass begins]", "[submitted]"), launches("[submitted]", "[pass ends]")


@pytest.mark.parametrize("mode", ("strip", "tile"))
def test_the_launches_of_a_bayer_pass(mode):
    ret2, status2, name2, few, slow2 = _trace(2, mode)
    ret8, status8, name8, many, slow8 = _trace(8, mode)
    assert (ret2, status2) == (2, [0] * 2) and (ret8, status8) == (8, [0] * 8)
    kernels = [k for k, _ in few]
    assert kernels == [k for k, _ in many], "the kernels of a pass depend on the number of samples"
    if mode == "strip":
        assert kernels.count("k_inv_bayer_strip") == 1 and "k_inv_packed16" not in kernels and "k_bayer_to_byr4" not in kernels, kernels
        assert name2 == name8 == "k_inv_bayer_strip"
    else:
        assert kernels.count("k_inv_packed16") == 1 and kernels.count("k_bayer_to_byr4") == 1 and "k_inv_bayer_strip" not in kernels, kernels
        assert kernels.index("k_inv_packed16") + 1 == kernels.index("k_bayer_to_byr4")
        assert name2 == name8 == "k_inv_packed16+k_bayer_to_byr4"
    for k in ("k_dec_ingest", "k_dec_parse", "k_dec_blank", "k_dec_lowpass"): assert kernels.count(k) == 1, k
    assert kernels[-1] == "k_dec_blank"
    # an intact pass: everything is launched by submit, wait launches nothing
    assert slow2 == [] and slow8 == []
    grew = 0
    for (k, a), (_, b) in zip(few, many):
        assert all(y >= x for x, y in zip(a, b)), (k, a, b)
        grew += a != b
    assert grew >= 5
    at = {k: g for k, g in many}
    assert at["k_dec_parse"][0] == 8 and at["k_dec_lowpass"][1] == 4 * 8
    # 192 x 96: a band of 48 x 24 -- one segment, two strips, a wave each: 2 waves a sample, four waves a workgroup
    if mode == "strip": assert at["k_inv_bayer_strip"] == (4, 1, 1) and dict(few)["k_inv_bayer_strip"] == (1, 1, 1)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(int(sys.argv[1]), sys.argv[2])
