"""tests/test_gpu_group_stream_batches.py on the CPU against the emulated product library (cfhd_testlib.emulated_product), and what only the emulator can show: the
launch trace of a pass (HIPEMU_TRACE, in a child process as tests/test_stream_batches_emulated.py does it) -- a pass of a group stream whose tables have settled, and a
pass of a group stream over a word whose tables never move, launch what a pass of cfhd_amd_batch_create_groups' batch of the same geometry launches: the same kernels
over the same grids."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import group_stream_batches as G
    pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")


    @pytest.mark.parametrize("route,quality", G.STREAM_CASES)
    def test_emulated_group_stream_equals_one_handle_and_the_reference(route, quality):
        with emulated_product():
            G.check_stream(route, quality)


    def test_emulated_group_stream_at_one_more_geometry():
        with emulated_product():
            G.check_other_geometry()


    def test_emulated_group_stream_pass_that_stands_still():
        with emulated_product():
            G.check_still_pass()


    @pytest.mark.parametrize("route", G.STATIC_CASES)
    def test_emulated_static_word_through_the_group_stream_entry(route):
        with emulated_product():
            G.check_static_word(route)


    def test_emulated_group_streams_on_the_queue():
        with emulated_product():
            G.check_queue()


    def test_emulated_group_stream_gates():
        with emulated_product():
            G.check_gates()
        G.host_entropy_child(True)


def _child(what, route, mode):
    """One batch of eight 192 x 96 frames and one traced pass: "still" -- a FILMSCAN2 group stream over copies of one frame, settled first --, "groups" -- FILMSCAN1
    (the only word create_groups takes here) over copies of the same frame --, "group_stream" / "groups-distinct" -- FILMSCAN1 over distinct frames through either
    entry.  The trace goes to stderr."""
    import cfhd_testlib as T
    import group_stream_batches as G
    fmt, w, interlaced, _, _ = G.ROUTES[route]
    with T.emulated_product():
        if what == "still":
            frames = [G.noisy_frame(fmt, w, G.H, 0, 6)] * G.N
            bt = G.Batch(w, G.H, fmt, interlaced, G.FILMSCAN2, G.N, mode)
            G.settle(bt, frames[0])
        else:
            frames = [G.noisy_frame(fmt, w, G.H, 0 if what == "groups" else i, 6) for i in range(G.N)]
            bt = G.Batch(w, G.H, fmt, interlaced, T.QUALITY_FILMSCAN1, G.N, mode, entry="group_stream" if what == "group_stream" else "groups")
            bt.feed(frames); bt.roundtrip()                 # (the traced pass is the second of either batch)
        bt.feed(frames)
        sys.stderr.write("[pass begins]\n"); sys.stderr.flush()
        assert bt.L.cfhd_amd_batch_submit(bt.b) == 0
        assert bt.L.cfhd_amd_batch_wait(bt.b) > 0, T.amd_last_error()
        sys.stderr.write("[pass ends]\n"); sys.stderr.flush()
        if what in ("still", "group_stream"): assert bt.stats() == (0, [1, G.N, 0]), bt.stats()
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


def test_a_settled_group_stream_pass_launches_what_a_create_groups_pass_launches():
    assert _trace("still", "YUY2", 1) == _trace("groups", "YUY2", 1)


@pytest.mark.parametrize("route", ["YUY2", "BGRA"])
def test_a_static_word_launches_the_same_through_either_group_entry(route):
    assert _trace("group_stream", route, 0) == _trace("groups-distinct", route, 0)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[1], sys.argv[2], int(sys.argv[3]))
