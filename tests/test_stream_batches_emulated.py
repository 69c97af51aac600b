"""tests/test_gpu_stream_batches.py on the CPU against the emulated product library (cfhd_testlib.emulated_product), and what only the emulator can show: the launch
trace of a pass (HIPEMU_TRACE, in a child process as tests/test_group_batches_rgb8_emulated.py does it) -- a pass of a stream whose tables have settled, and a pass of
a stream over a word whose tables never move, launch what a pass of cfhd_amd_batch_create_ex's batch of the same geometry launches: the same kernels over the same grids."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import stream_batches as S
    pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")


    @pytest.mark.parametrize("route,quality", S.STREAM_CASES)
    def test_emulated_stream_equals_one_handle_and_the_reference(route, quality):
        with emulated_product():
            S.check_stream(route, quality)


    def test_emulated_stream_pass_that_stands_still():
        with emulated_product():
            S.check_still_pass()


    @pytest.mark.parametrize("route", S.STATIC_CASES)
    def test_emulated_static_word_through_the_stream_entry(route):
        with emulated_product():
            S.check_static_word(route)


    def test_emulated_stream_batches_on_the_queue():
        with emulated_product():
            S.check_queue()


    def test_emulated_stream_batch_gates():
        with emulated_product():
            S.check_gates()
        S.host_entropy_child(True)


def _child(what, route, mode):
    """One batch of eight 192 x 96 frames and one traced pass: "still" -- a FILMSCAN2 stream over copies of one frame, settled first --, "stream" / "ex" -- FILMSCAN1
    through either entry.  The trace goes to stderr."""
    import cfhd_testlib as T
    import stream_batches as S
    fmt, enc, flags, _ = S.ROUTES[route]
    with T.emulated_product():
        if what == "still":
            frame = S.noisy_frame(fmt, S.W, S.H, 0, 6)
            bt = S.Batch(S.W, S.H, fmt, enc, flags, S.FILMSCAN2, S.N, mode)
            S.settle(bt, frame)
            frames = [frame] * S.N
        else:
            frames = [S.noisy_frame(fmt, S.W, S.H, i, 6) for i in range(S.N)]
            bt = S.Batch(S.W, S.H, fmt, enc, flags, T.QUALITY_FILMSCAN1, S.N, mode, entry=what)
            bt.feed(frames); bt.roundtrip()                 # (the traced pass is the second of either batch)
        bt.feed(frames)
        sys.stderr.write("[pass begins]\n"); sys.stderr.flush()
        assert bt.L.cfhd_amd_batch_submit(bt.b) == 0
        assert bt.L.cfhd_amd_batch_wait(bt.b) > 0, T.amd_last_error()
        sys.stderr.write("[pass ends]\n"); sys.stderr.flush()
        if what != "ex": assert bt.stats() == (0, [1, S.N, 0]), bt.stats()
        bt.close()


def _trace(what, route, mode):
    """[(kernel, grid)] of the traced pass."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), what, route, str(mode)], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stderr.splitlines()
    lines = lines[lines.index("[pass begins]") + 1: lines.index("[pass ends]")]
    launches = []
    for line in lines:
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
        if m: launches.append((m.group(1).rsplit("::", 1)[-1], (int(m.group(3)), int(m.group(4)), int(m.group(5)))))
    assert launches and any(k == "k_ent_emit" for k, _ in launches), lines[:20]
    return launches


def test_a_settled_stream_pass_launches_what_a_create_ex_pass_launches():
    assert _trace("still", "YUY2-422", 1) == _trace("ex", "YUY2-422", 1)


@pytest.mark.parametrize("route", ["YUY2-422", "RG48-444"])
def test_a_static_word_launches_the_same_through_either_entry(route):
    assert _trace("stream", route, 0) == _trace("ex", route, 0)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[1], sys.argv[2], int(sys.argv[3]))
