"""tests/test_gpu_device_pictures.py on the CPU against the emulated product library (cfhd_testlib.emulated_product: a device pointer is a host pointer), and what only
the CPU suite shows: the binary16 statement of the host-compiled build over all 65 536 words, from a stand-alone program built from the kernel's header (on the hardware
the same rule is the convert instruction, which the GPU suite checks), and the launch trace (HIPEMU_TRACE, in a child process) -- one k_dec_deliver behind k_dec_blank in a
pass that delivers, none once delivery is switched off."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import device_pictures as DP


    @pytest.mark.parametrize("name,kind,w,h,out,resolution,exact", DP.PACKED_CASES, ids=[c[0] for c in DP.PACKED_CASES])
    def test_emulated_packed_pictures_arrive_in_device_memory_and_nothing_else_is_touched(name, kind, w, h, out, resolution, exact):
        with emulated_product():
            DP.check_packed(name, kind, w, h, out, resolution, exact)


    @pytest.mark.parametrize("layout", [DP.PLANAR_U16, DP.PLANAR_F16, DP.PLANAR_F32], ids=["u16", "f16", "f32"])
    @pytest.mark.parametrize("name,kind,w,h,resolution", DP.PLANAR_CASES, ids=[c[0] for c in DP.PLANAR_CASES])
    def test_emulated_planar_tensors_equal_numpy_on_the_handles_words(name, kind, w, h, resolution, layout):
        with emulated_product():
            DP.check_planar(name, kind, w, h, resolution, layout)


    def test_the_host_compiled_binary16_rule_equals_numpy_on_every_word():
        DP.check_binary16_statement()


    @pytest.mark.parametrize("layout", [DP.PACKED, DP.PLANAR_F16], ids=["packed", "f16"])
    def test_emulated_device_memory_agrees_with_the_verdicts(layout):
        with emulated_product():
            DP.check_verdicts(layout)


    def test_emulated_a_short_pass_and_switching_off_leave_the_rest_alone():
        with emulated_product():
            DP.check_short_pass_and_off()


    def test_emulated_gates_and_the_kernel_time():
        with emulated_product():
            DP.check_gates()


    @pytest.mark.parametrize("name,negative_pitch", [("YUY2", False), ("RG48", False), ("YUY2 groups", False), ("YUY2", True)], ids=["yuy2", "rg48", "yuy2-groups", "yuy2-negative-pitch"])
    def test_emulated_frames_from_device_memory_encode_to_the_same_samples(name, negative_pitch):
        with emulated_product():
            DP.check_upload_device(name, negative_pitch)


    def test_emulated_decode_to_device_pictures_then_encode_from_them():
        with emulated_product():
            DP.check_chain()


def _child():
    """A pass that delivers, delivery switched off, a further pass: the trace of each -- submit to wait -- to stderr."""
    import cfhd_testlib as T
    import decode_queue as DQ
    import device_pictures as DP
    with T.emulated_product():
        samples = DQ.samples_of("422", 192, 96, DP.source())
        q = DQ.Queue(samples[0], "YU64", DQ.FULL, 8)
        d = DP.Delivery(q, DP.PACKED, True, 8); d.set()
        for k in range(2):
            sys.stderr.write("[pass %d begins]\n" % k); sys.stderr.flush()
            assert DP.run_pass(q, samples) == (8, [0] * 8)
            sys.stderr.write("[pass %d ends]\n" % k); sys.stderr.flush()
            assert DP.lib().cfhd_amd_decode_batch_set_device_pictures(q.b, None, 0, 0, 0) == 0
        q.close()
    print("TRACED")


def test_one_deliver_launch_behind_the_blank_and_none_once_switched_off():
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "trace"], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "TRACED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stderr.splitlines()
    def launches(k):
        out = []
        for line in lines[lines.index("[pass %d begins]" % k) + 1: lines.index("[pass %d ends]" % k)]:
            m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
            if m: out.append((m.group(1).rsplit("::", 1)[-1], tuple(int(m.group(j)) for j in (3, 4, 5))))
        return out
    first, second = launches(0), launches(1)
    names = [k for k, _ in first]
    assert names.count("k_dec_deliver") == 1 and names[-2:] == ["k_dec_blank", "k_dec_deliver"], names
    assert dict(first)["k_dec_deliver"][1] == 8, first[-1]            # (row pieces, pictures)
    # switched off: the pass launches exactly what it launched before it could deliver
    assert [k for k, _ in second] == names[:-1] and second == first[:-1], (first, second)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child()
