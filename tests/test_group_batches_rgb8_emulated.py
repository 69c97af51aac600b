"""tests/test_gpu_group_batches_rgb8.py on the CPU against the emulated product library (cfhd_testlib.emulated_product), and what only the emulator can show: the
launch trace of a pass (HIPEMU_TRACE, in a child process as tests/test_group_batches_emulated.py does it) -- a pass over groups from RG24 launches
k_ent_split_two_pass exactly once, a round trip also k_dec_band_two_pass exactly once, a pass over groups from YUY2 neither, through either constructor."""
import json, os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import group_batches_rgb8 as G8
    pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/libcfhd_ref.so is not built")


    @pytest.mark.parametrize("name,w,h,nframes,flash", G8.CASES)
    def test_emulated_rgb8_group_batch_samples_equal_the_reference(name, w, h, nframes, flash):
        with emulated_product():
            G8.check_samples(name, w, h, nframes, flash)


    @pytest.mark.parametrize("name,w,h", G8.HANDLE_CASES)
    def test_emulated_rgb8_group_handle_codes_on_the_device(name, w, h):
        with emulated_product():
            G8.check_handle(name, w, h)


    def test_emulated_rgb8_group_handle_with_rate_feedback():
        with emulated_product():
            G8.check_handle("RG24", 192, 96, quality=5, nframes=6)


    @pytest.mark.parametrize("name,w,h,nframes,flash", G8.ROUNDTRIP_CASES)
    def test_emulated_rgb8_group_batch_pictures(name, w, h, nframes, flash):
        with emulated_product():
            G8.check_pictures(name, w, h, nframes, flash)


    def test_emulated_rgb8_group_batches_on_the_queue():
        with emulated_product():
            G8.check_queue()


    def test_emulated_rgb8_group_batch_gates():
        with emulated_product():
            G8.check_gates()


def _child(name, mode, constructor):
    """One batch of four 192 x 96 frames and one queued pass; the trace goes to stderr."""
    import cfhd_testlib as T
    import group_batches as GB
    import group_batches_rgb8 as G8
    import gop_input_frames
    with T.emulated_product():
        if constructor == "groups":
            frames, pitch = GB.case_frames(192, 96, name, 0, 4) if name == "YUY2" else gop_input_frames.frames(name, 192, 96, 4)
            bt = G8.Batch(192, 96, name, 4, mode, frames, pitch)
        else: bt = GB.Batch(192, 96, name, 0, 4, mode)
        sys.stderr.write("[pass begins]\n"); sys.stderr.flush()
        assert bt.L.cfhd_amd_batch_submit(bt.b) == 0
        assert bt.L.cfhd_amd_batch_wait(bt.b) > 0, T.amd_last_error()
        sys.stderr.write("[pass ends]\n"); sys.stderr.flush()
        bt.close()


def _trace(name, mode, constructor):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(mode), constructor], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stderr.splitlines()
    lines = lines[lines.index("[pass begins]") + 1: lines.index("[pass ends]")]
    kernels = []
    for line in lines:
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
        if m: kernels.append(m.group(1).rsplit("::", 1)[-1])
    return kernels


def test_the_two_pass_kernels_launch_once_and_only_for_rgb8_groups():
    encode = _trace("RG24", 1, "groups")
    assert encode.count("k_ent_split_two_pass") == 1 and encode.count("k_dec_band_two_pass") == 0, encode
    assert encode.index("k_gop_quant_lowpass") < encode.index("k_ent_split_two_pass") < encode.index("k_ent_scan")
    roundtrip = _trace("RG24", 0, "groups")
    assert roundtrip.count("k_ent_split_two_pass") == 1 and roundtrip.count("k_dec_band_two_pass") == 1, roundtrip
    for constructor in ("groups", "ex"):
        yuy2 = _trace("YUY2", 0, constructor)
        assert "k_ent_emit" in yuy2 and "k_dec_parse_group" in yuy2
        assert yuy2.count("k_ent_split_two_pass") == 0 and yuy2.count("k_dec_band_two_pass") == 0, (constructor, yuy2)
    # every other launch of a YUY2 pass is what it was: the two constructors make the same batch
    assert _trace("YUY2", 0, "groups") == yuy2


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[1], int(sys.argv[2]), sys.argv[3])
