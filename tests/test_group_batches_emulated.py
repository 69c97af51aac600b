"""tests/test_gpu_group_batches.py on the CPU against the emulated product library (cfhd_testlib.emulated_product, as tests/test_group_outputs_emulated.py does), and
what only the emulator can show: the launch trace of a pass (HIPEMU_TRACE, in a child process as tests/test_launch_routes_emulated.py does it) -- the same sequence
of kernels for 2 groups and for 8, only the grids grow; the reported kernel names are the launched transform kernels in order; k_dec_parse_group once per pass.
(The emulator's trace has one line per kernel launch and none per synchronisation: that no host wait lies between a submit's first and last launch is shown by
reading gop_launch, not here.)"""
import ctypes, json, os, re, subprocess, sys
import numpy as np
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import group_batches as GB
    pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")


    @pytest.mark.parametrize("w,h,name,interlaced,nframes", GB.SAMPLE_CASES)
    def test_emulated_group_batch_samples_equal_the_c_abi_stream(w, h, name, interlaced, nframes):
        with emulated_product():
            GB.check_samples_equal_the_c_abi_stream(w, h, name, interlaced, nframes)


    @pytest.mark.parametrize("w,h,name,interlaced,nframes,flags", GB.PICTURE_CASES)
    def test_emulated_group_batch_pictures(w, h, name, interlaced, nframes, flags):
        with emulated_product():
            GB.check_pictures(w, h, name, interlaced, nframes, flags)


    def test_emulated_group_batches_on_the_queue():
        with emulated_product():
            GB.check_queue()


    def test_emulated_group_batch_gates():
        with emulated_product():
            GB.check_gates()

TRANSFORM = re.compile(r"k_(fwd|inv|gop|half|yu64)_")


def _child(nframes, name):
    """One round-trip batch of 192 x 96 frames, its six kernel names and one queued pass; names to stdout as JSON, the trace to stderr."""
    import cfhd_testlib as T
    import group_batches as GB
    with T.emulated_product():
        bt = GB.Batch(192, 96, name, 0, nframes, 0)
        names = [bt.L.cfhd_amd_batch_kernel_name(bt.b, slot).decode() for slot in range(6)]
        sys.stderr.write("[pass begins]\n"); sys.stderr.flush()
        assert bt.L.cfhd_amd_batch_submit(bt.b) == 0
        assert bt.L.cfhd_amd_batch_wait(bt.b) > 0, T.amd_last_error()
        sys.stderr.write("[pass ends]\n"); sys.stderr.flush()
        bt.close()
    print("NAMES " + json.dumps(names))


def _trace(nframes, name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(nframes), name], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    names = json.loads(next(line for line in run.stdout.splitlines() if line.startswith("NAMES "))[6:])
    lines = run.stderr.splitlines()
    lines = lines[lines.index("[pass begins]") + 1: lines.index("[pass ends]")]
    launches = []
    for line in lines:
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
        if m: launches.append((m.group(1).rsplit("::", 1)[-1], tuple(int(m.group(k)) for k in (3, 4, 5))))
    return names, launches


@pytest.mark.parametrize("name", ["YUY2", "RG48"])
def test_one_launch_per_stage_whatever_the_group_count(name):
    names2, few = _trace(4, name)
    names8, many = _trace(16, name)
    kernels = [k for k, _ in few]
    assert kernels == [k for k, _ in many], "the kernels of a pass depend on the number of groups"
    assert names2 == names8
    assert kernels.count("k_dec_parse_group") == 1
    for k in ("k_gop_temporal_fwd", "k_gop_temporal_inv", "k_dec_lowpass", "k_ent_emit"): assert kernels.count(k) == 1, k
    assert kernels.count("k_fwd_plane") == 2 and kernels.count("k_inv_plane") == 2
    # only the grids grow: no launch of the larger batch is smaller, the job dimension grows fourfold where it is the job index
    grew = 0
    for (k, a), (_, b) in zip(few, many):
        assert all(y >= x for x, y in zip(a, b)), (k, a, b)
        grew += a != b
    assert grew >= 8
    at = {k: g for k, g in many}
    assert at["k_gop_temporal_fwd"][1] == 3 * 8 and at["k_gop_temporal_inv"][1] == 3 * 8 and at["k_dec_parse_group"][0] == 8 and at["k_dec_lowpass"][1] == 6 * 8
    # the reported names, in launch order (slots 0, 1, 2, 5, 4, 3; "a+b": two launches), are the launched transform kernels
    reported = [k for slot in (0, 1, 2, 5, 4, 3) for k in names8[slot].split("+") if k]
    launched = [k for k in kernels if TRANSFORM.match(k)]
    print("reported", reported, "\nlaunched", launched)
    assert launched == reported


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(int(sys.argv[1]), sys.argv[2])
