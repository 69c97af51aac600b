"""tests/test_gpu_bayer_planes.py on the CPU against the emulated product library (cfhd_testlib.emulated_product: a device pointer is a host pointer), and what only the CPU
suite shows: the launch trace (HIPEMU_TRACE, in a child process) -- one k_dec_deliver_bayer behind k_dec_blank in a pass that delivers planes, its grid (pieces of quad
rows, pictures); one k_enc_collect_bayer per call with grid y = count and none in a pass; a Bayer decode pass with PACKED and a frame-queue pass never fed planes launch
exactly what batches that never saw the new layouts launch.  The element rules are the RG48 ones, whose host statements tests/test_device_pictures_emulated.py and
tests/test_planar_frames_emulated.py hold to numpy."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import bayer_planes as BP

    TWO = [BP.BAYER_U16, BP.BAYER_F32]


    @pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
    @pytest.mark.parametrize("w,h", BP.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in BP.GEOMETRY_SHAPES])
    def test_emulated_delivered_planes_equal_numpy_on_the_handles_mosaics(w, h, layout):
        with emulated_product():
            BP.check_delivery(w, h, layout)


    @pytest.mark.parametrize("layout", [BP.BAYER_F16, BP.BAYER_F32], ids=["f16", "f32"])
    def test_emulated_a_short_pass_touches_nothing_else_and_packed_and_null_switch_back(layout):
        with emulated_product():
            BP.check_short_pass_and_switching(layout)


    @pytest.mark.parametrize("layout", [BP.BAYER_U16, BP.BAYER_F16], ids=["u16", "f16"])
    def test_emulated_planes_agree_with_the_verdicts(layout):
        with emulated_product():
            BP.check_verdicts(layout)


    @pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
    def test_emulated_every_element_becomes_the_word_numpy_gives(layout):
        with emulated_product():
            BP.check_collection(layout)


    @pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
    def test_emulated_a_delivered_mosaic_comes_back(layout):
        with emulated_product():
            BP.check_inversion(layout)


    @pytest.mark.parametrize("layout", BP.LAYOUTS, ids=BP.LAYOUT_IDS)
    @pytest.mark.parametrize("w,h", BP.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in BP.GEOMETRY_SHAPES])
    def test_emulated_runs_of_frames_at_every_geometry_and_nothing_else_touched(w, h, layout):
        with emulated_product():
            BP.check_runs(w, h, layout)


    @pytest.mark.parametrize("layout", TWO, ids=["u16", "f32"])
    @pytest.mark.parametrize("kind", BP.KIND_IDS)
    def test_emulated_every_kind_of_byr4_batch_encodes_to_the_samples_of_the_uploaded_mosaics(kind, layout):
        with emulated_product():
            BP.check_kind(kind, layout)


    @pytest.mark.parametrize("layout", TWO, ids=["u16", "f32"])
    def test_emulated_decode_to_planes_then_encode_from_them(layout):
        with emulated_product():
            BP.check_chain(layout)


    def test_emulated_decode_queue_gates():
        with emulated_product():
            BP.check_decode_gates()


    def test_emulated_frame_queue_gates():
        with emulated_product():
            BP.check_frame_gates()


def _child():
    """Decode queue: batch A -- a pass into planes, a pass with PACKED --, batch B, which never saw a BAYER layout -- a pass with PACKED.  Frame queue: batch C -- frames
    uploaded from the host, frames 1 - 2 fed from planes, a pass, frames uploaded from the host, a pass --, batch D, never fed planes -- a pass.  The trace of each to
    stderr."""
    import numpy as np
    import cfhd_testlib as T
    import bayer_planes as BP
    import bayer_queue as BQ
    import device_pictures as DP
    def mark(text): sys.stderr.write("[%s]\n" % text); sys.stderr.flush()
    with T.emulated_product():
        w, h = 192, 96
        samples = BQ.samples_of(w, h, "amd")
        qa, qb = BQ.Queue(samples[0], 8), BQ.Queue(samples[0], 8)
        d = BP.Delivery(qa, BP.BAYER_F32, True, 8); d.set()
        mark("planes begins"); assert DP.run_pass(qa, samples, count=5) == (5, [0] * 5); mark("planes ends")
        pa = DP.Delivery(qa, DP.PACKED, True, 8); pa.set()
        mark("packed a begins"); assert DP.run_pass(qa, samples, count=5) == (5, [0] * 5); mark("packed a ends")
        pb = DP.Delivery(qb, DP.PACKED, True, 8); pb.set()
        mark("packed b begins"); assert DP.run_pass(qb, samples, count=5) == (5, [0] * 5); mark("packed b ends")
        qa.close(); qb.close()
        planes = BP.geometry_frames(w, h, BP.BAYER_F32)
        mosaics = [BP.collected(f, BP.BAYER_F32) for f in planes]
        src = BP.Source(planes, w, h, BP.BAYER_F32, True)
        with BP.Batch(BP.EX, w, h, 4) as c, BP.Batch(BP.EX, w, h, 4) as e:
            c.upload(mosaics[::-1], 2 * w)
            mark("call begins"); src.feed(c.L, c.b, 1, 2); mark("call ends")
            mark("pass c1 begins"); first = c.run(); mark("pass c1 ends")
            c.upload(mosaics, 2 * w)
            mark("pass c2 begins"); second = c.run(); mark("pass c2 ends")
            e.upload(mosaics, 2 * w)
            mark("pass d begins"); third = e.run(); mark("pass d ends")
            assert len(first) == 4 and len(second) == 4 and len(third) == 4
    print("TRACED")


def test_one_launch_of_each_new_kernel_where_it_belongs_and_none_elsewhere():
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
    planes, packed_a, packed_b = launches("planes"), launches("packed a"), launches("packed b")
    names = [k for k, _ in planes]
    assert names.count("k_dec_deliver_bayer") == 1 and names[-2:] == ["k_dec_blank", "k_dec_deliver_bayer"] and "k_dec_deliver" not in names, names
    assert planes[-1][1] == (12, 5, 1), planes[-1]                      # (dec_deliver_pieces(48 quad rows): four a piece; the pictures of the pass)
    assert [k for k, _ in packed_b][-2:] == ["k_dec_blank", "k_dec_deliver"] and "k_dec_deliver_bayer" not in [k for k, _ in packed_b], packed_b
    assert packed_a == packed_b and planes[:-1] == packed_b[:-1], (planes, packed_a, packed_b)
    call, c1, c2, d = launches("call"), launches("pass c1"), launches("pass c2"), launches("pass d")
    assert call == [("k_enc_collect_bayer", (12, 2, 1))], call         # (enc_collect_pieces(48 quad rows); frames)
    assert len(d) >= 4 and not [k for k, _ in d if k.startswith("k_enc_collect")], d
    assert c1 == d and c2 == d, (c1, c2, d)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child()
