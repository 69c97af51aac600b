"""tests/test_gpu_planar_frames.py on the CPU against the emulated product library (cfhd_testlib.emulated_product: a device pointer is a host pointer), and what only the
CPU suite shows: the host statement of the element rules over all binary16 patterns and the float32 set of the rule test, from a stand-alone program built from the
kernel's header (on the hardware the same rules are the convert and round instructions, which the GPU suite checks), and the launch trace (HIPEMU_TRACE, in a child
process) -- one k_enc_collect per call with grid y = count, none in a pass, and a pass of a batch that was fed planar launches what a batch that never was launches."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import planar_frames as PF


    @pytest.mark.parametrize("layout", PF.LAYOUTS, ids=PF.LAYOUT_IDS)
    def test_emulated_every_element_becomes_the_word_numpy_gives(layout):
        with emulated_product():
            PF.check_word_rule(layout)


    @pytest.mark.parametrize("layout", [PF.PLANAR_U16, PF.PLANAR_F32], ids=["u16", "f32"])
    def test_emulated_a_delivered_picture_comes_back_word_for_word(layout):
        with emulated_product():
            PF.check_delivery_is_inverted(layout)


    @pytest.mark.parametrize("layout", PF.LAYOUTS, ids=PF.LAYOUT_IDS)
    @pytest.mark.parametrize("w,h", PF.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in PF.GEOMETRY_SHAPES])
    def test_emulated_runs_of_frames_at_both_geometries_and_nothing_else_touched(w, h, layout):
        with emulated_product():
            PF.check_geometry(w, h, layout)


    @pytest.mark.parametrize("layout", [PF.PLANAR_U16, PF.PLANAR_F32], ids=["u16", "f32"])
    @pytest.mark.parametrize("kind,mode", PF.KIND_CASES, ids=PF.KIND_IDS)
    def test_emulated_every_kind_of_batch_encodes_to_the_samples_of_the_packed_frames(kind, mode, layout):
        with emulated_product():
            PF.check_kind(kind, mode, layout)


    def test_emulated_a_run_across_the_chunks_of_a_batch():
        with emulated_product():
            PF.check_chunks()


    @pytest.mark.parametrize("layout", PF.LAYOUTS, ids=PF.LAYOUT_IDS)
    def test_emulated_decode_to_planar_pictures_then_encode_from_them(layout):
        with emulated_product():
            PF.check_chain(layout)


    def test_emulated_gates():
        with emulated_product():
            PF.check_gates()


    def test_emulated_download_frame_of_other_inputs():
        with emulated_product():
            PF.check_download_frame_of_other_inputs()


    def test_the_host_compiled_rules_equal_numpy():
        PF.check_host_statement()


def _child():
    """Batch A: frames uploaded from the host, frames 1 - 2 fed planar, a pass, frames uploaded from the host, a pass.  Batch B: never fed planar, a pass.  The trace of
    the call and of each pass to stderr."""
    import numpy as np
    import cfhd_testlib as T
    import planar_frames as PF
    def mark(text): sys.stderr.write("[%s]\n" % text); sys.stderr.flush()
    with T.emulated_product():
        w, h = 192, 96
        planes = PF.geometry_frames(w, h, PF.PLANAR_F32)
        packed = [PF.packed_frame(PF.expected_words(f, PF.PLANAR_F32)) for f in planes]
        src = PF.Source(planes, w, h, PF.PLANAR_F32, True)
        with PF.Batch(PF.RG48_444, w, h, 4) as a, PF.Batch(PF.RG48_444, w, h, 4) as b:
            a.upload(packed[::-1], 6 * w)
            mark("call begins"); src.feed(a.L, a.b, 1, 2); mark("call ends")
            mark("pass a1 begins"); first = a.run(); mark("pass a1 ends")
            a.upload(packed, 6 * w)
            mark("pass a2 begins"); second = a.run(); mark("pass a2 ends")
            b.upload(packed, 6 * w)
            mark("pass b begins"); third = b.run(); mark("pass b ends")
            assert len(first) == 4 and len(second) == 4 and len(third) == 4
    print("TRACED")


def test_one_collect_launch_per_call_and_none_in_a_pass():
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
    call, a1, a2, b = launches("call"), launches("pass a1"), launches("pass a2"), launches("pass b")
    assert call == [("k_enc_collect", (24, 2, 1))], call              # (row pieces: 96 rows, four a piece; frames)
    assert len(b) >= 4 and "k_enc_collect" not in [k for k, _ in b], b
    # the pass of a batch that was fed planar -- in front of this pass, and in front of the pass before -- launches exactly what a batch that never was launches
    assert a1 == b and a2 == b, (a1, a2, b)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child()
