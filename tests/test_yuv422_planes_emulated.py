"""tests/test_gpu_yuv422_planes.py on the CPU against the emulated product library (cfhd_testlib.emulated_product: a device pointer is a host pointer), and what only
the CPU suite shows: the host-compiled statement of the element rules at both units against numpy, and the launch trace (HIPEMU_TRACE, in a child process) -- one
k_dec_deliver_yuv422 behind k_dec_blank in a pass that delivers planes, its grid (row pieces, pictures); one k_enc_collect_yuv422 per call with grid y = count and
none in a pass; a decode pass with PACKED and a frame-queue pass never fed planes launch exactly what batches that never saw the new layouts launch."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import yuv422_planes as YP
    from decode_queue import FULL, HALF

    FORMAT_LAYOUTS = [(f, l) for f in YP.FORMATS for l in YP.layouts_of(f)]
    FORMAT_LAYOUT_IDS = ["%s-%s" % (f, YP.LAYOUT_NAMES[l]) for f, l in FORMAT_LAYOUTS]
    CHAIN = [("YUY2", YP.YUV422_U8), ("YUY2", YP.YUV422_F16), ("YUY2", YP.YUV422_F32), ("YU64", YP.YUV422_U16), ("YU64", YP.YUV422_F32)]
    CHAIN_IDS = ["%s-%s" % (f, YP.LAYOUT_NAMES[l]) for f, l in CHAIN]
    DELIVERIES = [("422",) + s + (FULL,) for s in YP.GEOMETRY_SHAPES + [YP.LONG32]] + [("422",) + YP.HALF_OF + (HALF,)]
    DELIVERY_IDS = ["%dx%d%s" % (w, h, "-half" if r == HALF else "") for _, w, h, r in DELIVERIES]
    OTHER_KINDS = [("422i", "YUY2", FULL), ("422i", "2vuy", HALF), ("groups", "YU64", FULL), ("groups", "YUY2", HALF), ("groups-i", "2vuy", FULL)]


    def test_the_host_compiled_rules_equal_numpy_at_both_units_and_invert():
        YP.check_host_statement()


    @pytest.mark.parametrize("fmt", YP.FORMATS)
    @pytest.mark.parametrize("kind,w,h,resolution", DELIVERIES, ids=DELIVERY_IDS)
    def test_emulated_delivered_planes_equal_numpy_on_the_pass_own_pictures(kind, w, h, resolution, fmt):
        with emulated_product():
            YP.check_delivery(kind, w, h, fmt, resolution)


    @pytest.mark.parametrize("kind,fmt,resolution", OTHER_KINDS, ids=["%s-%s%s" % (k, f, "-half" if r == HALF else "") for k, f, r in OTHER_KINDS])
    def test_emulated_interlaced_samples_and_groups_deliver_planes(kind, fmt, resolution):
        with emulated_product():
            YP.check_delivery(kind, 192, 96, fmt, resolution)


    @pytest.mark.parametrize("fmt,layout", [("YUY2", YP.YUV422_F16), ("YU64", YP.YUV422_U16)], ids=["YUY2-f16", "YU64-u16"])
    def test_emulated_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(fmt, layout):
        with emulated_product():
            YP.check_short_pass_and_switching(fmt, layout)


    @pytest.mark.parametrize("fmt,layout", [("YUY2", YP.YUV422_U8), ("YU64", YP.YUV422_F16), ("2vuy", YP.YUV422_F32)], ids=["YUY2-u8", "YU64-f16", "2vuy-f32"])
    def test_emulated_planes_agree_with_the_verdicts(fmt, layout):
        with emulated_product():
            YP.check_verdicts(fmt, layout)


    @pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
    def test_emulated_every_element_becomes_the_word_numpy_gives(fmt, layout):
        with emulated_product():
            YP.check_collection(fmt, layout)


    @pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
    def test_emulated_a_delivered_picture_comes_back(fmt, layout):
        with emulated_product():
            YP.check_inversion(fmt, layout)


    @pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
    @pytest.mark.parametrize("w,h", YP.GEOMETRY_SHAPES, ids=["%dx%d" % s for s in YP.GEOMETRY_SHAPES])
    def test_emulated_runs_of_frames_at_every_geometry_and_nothing_else_touched(w, h, fmt, layout):
        with emulated_product():
            YP.check_runs(fmt, w, h, layout)


    @pytest.mark.parametrize("kind", YP.KIND_IDS)
    def test_emulated_every_kind_of_422_batch_encodes_to_the_samples_of_the_uploaded_frames(kind):
        with emulated_product():
            YP.check_kind(kind)


    @pytest.mark.parametrize("kind", ["ex-2vuy-mode1", "groups-yu64"])
    def test_emulated_batches_fed_float_planes_encode_to_the_same_samples(kind):
        with emulated_product():
            YP.check_kind(kind, YP.YUV422_F32)


    @pytest.mark.parametrize("fmt,layout", CHAIN, ids=CHAIN_IDS)
    def test_emulated_decode_to_planes_then_collect_gives_the_packed_picture(fmt, layout):
        with emulated_product():
            YP.check_chain(fmt, layout)


    def test_emulated_decode_queue_gates():
        with emulated_product():
            YP.check_decode_gates()


    def test_emulated_frame_queue_gates():
        with emulated_product():
            YP.check_frame_gates()


def _child():
    """Decode queue: batch A -- a pass into planes, a pass with PACKED --, batch B, which never saw a YUV422 layout -- a pass with PACKED.  Frame queue: batch C -- frames
    uploaded from the host, frames 1 - 2 fed from planes, a pass, frames uploaded from the host, a pass --, batch D, never fed planes -- a pass.  The trace of each to
    stderr."""
    import cfhd_testlib as T
    import yuv422_planes as YP
    import decode_queue as DQ
    import device_pictures as DP
    def mark(text): sys.stderr.write("[%s]\n" % text); sys.stderr.flush()
    with T.emulated_product():
        w, h = 192, 96
        samples = DQ.samples_of("422", w, h, "amd")
        qa, qb = DQ.Queue(samples[0], "YUY2", DQ.FULL, 8), DQ.Queue(samples[0], "YUY2", DQ.FULL, 8)
        d = YP.Delivery(qa, "YUY2", YP.YUV422_F32, True, 8); d.set()
        mark("planes begins"); assert DP.run_pass(qa, samples, count=5) == (5, [0] * 5); mark("planes ends")
        pa = DP.Delivery(qa, DP.PACKED, True, 8); pa.set()
        mark("packed a begins"); assert DP.run_pass(qa, samples, count=5) == (5, [0] * 5); mark("packed a ends")
        pb = DP.Delivery(qb, DP.PACKED, True, 8); pb.set()
        mark("packed b begins"); assert DP.run_pass(qb, samples, count=5) == (5, [0] * 5); mark("packed b ends")
        qa.close(); qb.close()
        planes = YP.geometry_frames("YUY2", w, h, YP.YUV422_F32)
        packed = [YP.collected(f, "YUY2", YP.YUV422_F32) for f in planes]
        src = YP.Source(planes, w, h, YP.YUV422_F32, True)
        with YP.Batch(YP.intra("YUY2"), w, h, 4) as c, YP.Batch(YP.intra("YUY2"), w, h, 4) as e:
            c.upload(packed[::-1], 2 * w)
            mark("call begins"); src.feed(c.L, c.b, 1, 2); mark("call ends")
            mark("pass c1 begins"); first = c.run(); mark("pass c1 ends")
            c.upload(packed, 2 * w)
            mark("pass c2 begins"); second = c.run(); mark("pass c2 ends")
            e.upload(packed, 2 * w)
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
    assert names.count("k_dec_deliver_yuv422") == 1 and names[-2:] == ["k_dec_blank", "k_dec_deliver_yuv422"] and "k_dec_deliver" not in names, names
    assert planes[-1][1] == (24, 5, 1), planes[-1]                      # (dec_deliver_pieces(96 rows): four a piece; the pictures of the pass)
    assert [k for k, _ in packed_b][-2:] == ["k_dec_blank", "k_dec_deliver"] and "k_dec_deliver_yuv422" not in [k for k, _ in packed_b], packed_b
    assert packed_a == packed_b and planes[:-1] == packed_b[:-1], (planes, packed_a, packed_b)
    call, c1, c2, d = launches("call"), launches("pass c1"), launches("pass c2"), launches("pass d")
    assert call == [("k_enc_collect_yuv422", (24, 2, 1))], call         # (enc_collect_pieces(96 rows); frames)
    assert len(d) >= 4 and not [k for k, _ in d if k.startswith("k_enc_collect")], d
    assert c1 == d and c2 == d, (c1, c2, d)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child()
