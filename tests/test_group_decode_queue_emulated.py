"""tests/test_gpu_group_decode_queue.py on the CPU against the emulated product library (cfhd_testlib.emulated_product), and what only the emulator can show: the
launch trace of a pass of groups (HIPEMU_TRACE, in a child process) -- the same kernels for 1 group and for 8, only the grids grow; k_dec_ingest, k_dec_parse_group,
k_dec_band_two_pass, k_dec_lowpass and k_dec_blank once each; no launch in wait for an intact pass, the handle's launches behind a pass with a damaged code stream."""
import json, os, re, subprocess, sys
import numpy as np
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import group_decode_queue as GQ
    needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")
    SOURCES = [pytest.param("ref", marks=needs_ref), "amd"]


    @pytest.mark.parametrize("source", SOURCES)
    @pytest.mark.parametrize("interlaced,w,h,out,resolution", GQ.EXACT_CASES)
    def test_emulated_foreign_groups_decode_to_the_handles_pictures(interlaced, w, h, out, resolution, source):
        with emulated_product():
            GQ.check_foreign_exact(interlaced, w, h, out, resolution, source)


    @pytest.mark.parametrize("source", SOURCES)
    @pytest.mark.parametrize("interlaced,w,h,out,exact_out", GQ.DITHER_CASES)
    def test_emulated_dithered_outputs_stay_within_one_step_of_the_handle(interlaced, w, h, out, exact_out, source):
        with emulated_product():
            GQ.check_foreign_dithered(interlaced, w, h, out, exact_out, source)


    @pytest.mark.parametrize("source", SOURCES)
    @pytest.mark.parametrize("pix,w,h", GQ.TWO_PASS_CASES)
    def test_emulated_the_two_pass_band_is_decoded_on_the_device(pix, w, h, source):
        with emulated_product():
            GQ.check_two_pass_on_the_device(pix, w, h, source)


    @pytest.mark.parametrize("source", SOURCES)
    def test_emulated_one_pass_mixes_qualities(source):
        with emulated_product():
            GQ.check_mixed_qualities(source)


    @pytest.mark.parametrize("source", SOURCES)
    def test_emulated_one_pass_mixes_raw_word_and_two_pass_groups(source):
        with emulated_product():
            GQ.check_mixed_band_kinds(source)


    @pytest.mark.parametrize("source", SOURCES)
    def test_emulated_ingest_from_plain_registered_and_device_memory(source):
        with emulated_product():
            GQ.check_ingest(source)


    @pytest.mark.parametrize("source", SOURCES)
    def test_emulated_a_short_pass_leaves_the_rest_alone(source):
        with emulated_product():
            GQ.check_short_pass(source)


    @pytest.mark.parametrize("source", SOURCES)
    @pytest.mark.parametrize("kind,follower_kind", [(k, GQ.FOLLOWER_KINDS[i % 3]) for i, k in enumerate(GQ.VERDICT_KINDS)])
    def test_emulated_verdict_per_pair(kind, follower_kind, source):
        with emulated_product():
            GQ.check_verdicts(kind, follower_kind, source)


    def test_emulated_a_sequence_header_passed_as_a_sample_has_a_zero_picture():
        with emulated_product():
            GQ.check_sequence_header_as_a_sample()


    @pytest.mark.parametrize("source", SOURCES)
    def test_emulated_two_group_batches_in_flight(source):
        with emulated_product():
            GQ.check_queue(source)


    def test_emulated_gates():
        with emulated_product():
            GQ.check_gates()


    def test_emulated_gate_under_host_entropy():
        env = dict(os.environ, CFHD_AMD_ENTROPY="host")
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "host-entropy"], env=env, capture_output=True, text=True, timeout=900)
        assert run.returncode == 0 and "HOST ENTROPY REFUSED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def _child(ngroups, pix, damage):
    """One batch of 320 x 240 groups of the product's encoder and one pass; the trace of the pass -- submit to wait -- to stderr."""
    import cfhd_testlib as T
    import group_decode_queue as GQ
    with T.emulated_product():
        eight = GQ.group_stream("amd", 320, 240, pix=pix)
        samples = [eight[i % 8] for i in range(2 * ngroups)]
        if damage: samples[2], _ = GQ.damaged_group("payload pattern", samples[2], None)
        q = GQ.GroupQueue(eight[0], "YU64", GQ.FULL, ngroups)
        blob, offsets, sizes = GQ.pack(samples)
        sys.stderr.write("[pass begins]\n"); sys.stderr.flush()
        assert q.submit(blob, offsets, sizes) == 0, T.amd_last_error()
        sys.stderr.write("[submitted]\n"); sys.stderr.flush()
        ret, status = q.wait(2 * ngroups)
        sys.stderr.write("[pass ends]\n"); sys.stderr.flush()
        q.close()
    print("STATUS " + json.dumps([ret, status]))


def _trace(ngroups, pix="YUY2", damage=False):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(ngroups), pix, str(int(damage))], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ret, status = json.loads(next(line for line in run.stdout.splitlines() if line.startswith("STATUS "))[7:])
    lines = run.stderr.splitlines()
    def launches(a, b):
        out = []
        for line in lines[lines.index(a) + 1: lines.index(b)]:
            m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
            if m: out.append((m.group(1).rsplit("::", 1)[-1], tuple(int(m.group(k)) for k in (3, 4, 5))))
        return out
    return ret, status, launches("[pass begins]", "[submitted]"), launches("[submitted]", "[pass ends]")


def test_one_launch_per_stage_whatever_the_group_count():
    ret1, status1, few, slow1 = _trace(1)
    ret8, status8, many, slow8 = _trace(8)
    assert (ret1, status1) == (2, [0] * 2) and (ret8, status8) == (16, [0] * 16)
    kernels = [k for k, _ in few]
    assert kernels == [k for k, _ in many], "the kernels of a pass depend on the number of groups"
    for k in ("k_dec_ingest", "k_dec_parse_group", "k_dec_band_two_pass", "k_dec_lowpass", "k_dec_blank"): assert kernels.count(k) == 1, k
    assert kernels.index("k_dec_ingest") < kernels.index("k_dec_parse_group") and kernels[-1] == "k_dec_blank"
    assert slow1 == [] and slow8 == [], "an intact pass launches nothing in wait"
    grew = 0
    for (k, a), (_, b) in zip(few, many):
        assert all(y >= x for x, y in zip(a, b)), (k, a, b)
        grew += a != b
    assert grew >= 5
    at = {k: g for k, g in many}
    assert at["k_dec_parse_group"][0] == 8 and at["k_dec_band_two_pass"][0] == 3 * 8 and at["k_dec_blank"][1] == 16 and at["k_dec_lowpass"][1] == 6 * 8


def test_the_two_pass_kernel_runs_in_submit_and_wait_launches_nothing():
    ret, status, fast, slow = _trace(4, pix="RG24")
    assert (ret, status) == (8, [0] * 8)
    assert [k for k, _ in fast].count("k_dec_band_two_pass") == 1 and slow == []


def test_a_damaged_code_stream_sends_the_pass_through_the_handle():
    ret, status, fast, slow = _trace(4, damage=True)
    assert [k for k, _ in fast].count("k_dec_parse_group") == 1
    if ret == 8 and not slow: pytest.fail("the pattern left the code stream decodable: choose another")
    names = [k for k, _ in slow]
    assert names and "k_dec_ingest" not in names and names.count("k_dec_lowpass") >= 4, names


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "host-entropy":
        import cfhd_testlib as T
        import group_decode_queue as GQ
        with T.emulated_product():
            GQ.gates_under_host_entropy()
    else:
        _child(int(sys.argv[1]), sys.argv[2], int(sys.argv[3]))
