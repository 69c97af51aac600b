"""tests/test_gpu_rgb_as_yuv.py on the CPU against the emulated product library (cfhd_testlib.emulated_product: a device pointer is a host pointer; the kernel's
arithmetic host-compiled), and what only the CPU suite shows: the launch trace (HIPEMU_TRACE, in a child process) -- one k_dec_deliver_rgb_as_yuv behind k_dec_blank in
a pass that delivers an RGB_AS layout, its grid (row pieces, pictures), one more per run of handle-decoded samples of one matrix; passes with PACKED or PLANAR_*
launch exactly what batches that never saw the new layouts launch."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import rgb_as_yuv as RY

    LAYOUT_IDS = [RY.LAYOUT_NAMES[l] for l in RY.LAYOUTS]


    @pytest.mark.parametrize("name", RY.DELIVERY_IDS)
    def test_emulated_delivery_equals_the_model_on_the_pass_own_pictures_and_the_reference(name):
        with emulated_product():
            RY.check_delivery(name)


    @pytest.mark.parametrize("layout", [RY.RGB_AS_YU64, RY.RGB_AS_YUV422_F16], ids=["yu64", "f16"])
    def test_emulated_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(layout):
        with emulated_product():
            RY.check_short_pass_and_switching(layout)


    @pytest.mark.parametrize("layout", RY.LAYOUTS, ids=LAYOUT_IDS)
    def test_emulated_a_mixed_pass_converts_every_picture_with_the_matrix_of_its_own_sample(layout):
        with emulated_product():
            RY.check_mixed_pass(layout)


    @pytest.mark.parametrize("layout", RY.LAYOUTS, ids=LAYOUT_IDS)
    def test_emulated_a_failed_sample_is_zeros_and_its_neighbours_are_intact(layout):
        with emulated_product():
            RY.check_failed_samples(layout)


    @pytest.mark.parametrize("layout", [RY.RGB_AS_YU64, RY.RGB_AS_YUV422_U16], ids=["yu64", "u16"])
    def test_emulated_both_submit_paths_deliver_and_host_delivery_is_unchanged_beside_it(layout):
        with emulated_product():
            RY.check_submit_paths(layout)


    def test_emulated_gates():
        with emulated_product():
            RY.check_gates()


def _child():
    """Batch A: a pass of intact samples into planes, the mixed pass into the packed form, a pass with PLANAR_U16, a pass with PACKED.  Batch B, which never saw an RGB_AS
    layout: the same two last passes.  The trace of each to stderr."""
    import cfhd_testlib as T
    import rgb_as_yuv as RY
    import decode_queue as DQ
    import device_pictures as DP
    def mark(text): sys.stderr.write("[%s]\n" % text); sys.stderr.flush()
    with T.emulated_product():
        plain, mixed, _ = RY.mixed_pass()
        qa, qb = DQ.Queue(plain[0], "RG48", DQ.FULL, 8), DQ.Queue(plain[0], "RG48", DQ.FULL, 8)
        d = RY.Delivery(qa, RY.RGB_AS_YUV422_F32, True, 8); d.set()
        mark("planes begins"); assert RY.run_pass(qa, plain, count=5) == (5, [0] * 5); mark("planes ends")
        d2 = RY.Delivery(qa, RY.RGB_AS_YU64, True, 8); d2.set()
        mark("mixed begins"); assert RY.run_pass(qa, mixed) == (8, [0] * 8); mark("mixed ends")
        for q, name in ((qa, "a"), (qb, "b")):
            u16 = DP.Delivery(q, DP.PLANAR_U16, True, 8); u16.set()
            mark("planar %s begins" % name); assert RY.run_pass(q, plain, count=5) == (5, [0] * 5); mark("planar %s ends" % name)
            packed = DP.Delivery(q, DP.PACKED, True, 8); packed.set()
            mark("packed %s begins" % name); assert RY.run_pass(q, plain, count=5) == (5, [0] * 5); mark("packed %s ends" % name)
        qa.close(); qb.close()
    print("TRACED")


def test_one_launch_of_the_new_kernel_per_pass_one_more_per_run_of_handle_decoded_samples_and_none_elsewhere():
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "trace"], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "TRACED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stderr.splitlines()
    def launches(name):
        out = []
        for line in lines[lines.index("[%s begins]" % name) + 1: lines.index("[%s ends]" % name)]:
            m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
            if m: out.append((m.group(1).rsplit("::", 1)[-1], tuple(int(m.group(j)) for j in (3, 4, 5))))
        return out
    NEW = "k_dec_deliver_rgb_as_yuv"
    planes, mixed = launches("planes"), launches("mixed")
    names = [k for k, _ in planes]
    assert names.count(NEW) == 1 and names[-2:] == ["k_dec_blank", NEW] and "k_dec_deliver" not in names, names
    assert planes[-1][1] == (24, 5, 1), planes[-1]                      # (dec_deliver_pieces(96 rows): four a piece; the pictures of the pass)
    # the mixed pass: the launch of the pass over all eight pictures behind k_dec_blank, then, inside wait, one launch per run of handle-decoded samples: 1 - 2 and 5
    names = [k for k, _ in mixed]
    at = names.index("k_dec_blank")
    assert names[at + 1] == NEW and mixed[at + 1][1] == (24, 8, 1), mixed[at:]
    assert [(k, g) for k, g in mixed[at + 2:] if k == NEW] == [(NEW, (24, 2, 1)), (NEW, (24, 1, 1))] and names.count(NEW) == 3 and "k_dec_deliver" not in names, mixed[at:]
    for kind in ("planar", "packed"):
        a, b = launches("%s a" % kind), launches("%s b" % kind)
        assert [k for k, _ in b][-2:] == ["k_dec_blank", "k_dec_deliver"] and NEW not in [k for k, _ in b], b
        assert a == b, (kind, a, b)
    assert planes[:-1] == launches("packed b")[:-1], (planes, launches("packed b"))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child()
