"""tests/test_gpu_rgba_planes.py on the CPU against the emulated product library (cfhd_testlib.emulated_product: a device pointer is a host pointer; the element rules
host-compiled), and what only the CPU suite shows: the launch trace (HIPEMU_TRACE, in a child process) -- one k_dec_deliver_rgba behind k_dec_blank in a pass that
delivers planes, its grid (row pieces, pictures); one k_enc_collect_rgba per call with grid y = count, one per chunk of a cut batch, and none in a pass; a decode pass
with PACKED and a frame-queue pass never fed planes launch exactly what batches that never saw the new layouts launch."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import rgba_planes as RP

    FORMAT_LAYOUTS = [(f, l) for f in RP.FORMATS for l in RP.layouts_of(f)]
    FORMAT_LAYOUT_IDS = ["%s-%s" % (f, RP.LAYOUT_NAMES[l]) for f, l in FORMAT_LAYOUTS]
    CHAIN = [("b64a", RP.RGBA_U16), ("b64a", RP.RGBA_F16), ("b64a", RP.RGBA_F32), ("BGRA", RP.RGBA_U8), ("BGRA", RP.RGBA_F16), ("BGRa", RP.RGBA_F32)]
    CHAIN_IDS = ["%s-%s" % (f, RP.LAYOUT_NAMES[l]) for f, l in CHAIN]


    @pytest.mark.parametrize("name", RP.DECODE_IDS)
    def test_emulated_delivered_planes_equal_numpy_on_the_pass_own_pictures(name):
        with emulated_product():
            RP.check_delivery(name)


    @pytest.mark.parametrize("fmt,layout", [("b64a", RP.RGBA_F16), ("BGRA", RP.RGBA_U8)], ids=["b64a-f16", "BGRA-u8"])
    def test_emulated_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(fmt, layout):
        with emulated_product():
            RP.check_short_pass_and_switching(fmt, layout)


    @pytest.mark.parametrize("fmt,layout", [("b64a", RP.RGBA_F16), ("BGRA", RP.RGBA_U8), ("BGRa", RP.RGBA_F32)], ids=["b64a-f16", "BGRA-u8", "BGRa-f32"])
    def test_emulated_planes_agree_with_the_verdicts(fmt, layout):
        with emulated_product():
            RP.check_verdicts(fmt, layout)


    @pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
    def test_emulated_every_element_becomes_the_word_numpy_gives(fmt, layout):
        with emulated_product():
            RP.check_collection(fmt, layout)


    @pytest.mark.parametrize("fmt,layout", FORMAT_LAYOUTS, ids=FORMAT_LAYOUT_IDS)
    def test_emulated_a_delivered_picture_comes_back(fmt, layout):
        with emulated_product():
            RP.check_inversion(fmt, layout)


    @pytest.mark.parametrize("kind", RP.KIND_IDS)
    def test_emulated_every_kind_of_batch_takes_the_planes_and_encodes_to_the_samples_of_the_uploaded_frames(kind):
        with emulated_product():
            RP.check_kind(kind)


    def test_emulated_a_stream_fed_planes_for_two_passes_equals_the_stream_fed_packed_frames():
        with emulated_product():
            RP.check_stream()


    @pytest.mark.parametrize("fmt,layout", CHAIN, ids=CHAIN_IDS)
    def test_emulated_decode_to_planes_then_collect_gives_the_packed_picture(fmt, layout):
        with emulated_product():
            RP.check_chain(fmt, layout)


    def test_emulated_decode_queue_gates():
        with emulated_product():
            RP.check_decode_gates()


    def test_emulated_frame_queue_gates():
        with emulated_product():
            RP.check_frame_gates()


def _child():
    """Decode queue: batch A -- a pass into planes, a pass with PACKED --, batch B, which never saw an RGBA layout -- a pass with PACKED.  Frame queue: batch C -- frames
    uploaded from the host, frames 1 - 2 fed from planes, a pass, frames uploaded from the host, a pass --, batch D, never fed planes -- a pass --, and batch E, cut
    into chunks of three frames -- frames 1 - 3 fed from planes, a run across the cut.  The trace of each to stderr."""
    import cfhd_testlib as T
    import rgba_planes as RP
    import decode_queue as DQ
    import device_pictures as DP
    def mark(text): sys.stderr.write("[%s]\n" % text); sys.stderr.flush()
    with T.emulated_product():
        w, h = RP.SHAPE
        samples = DQ.samples_of("4444", w, h, "amd")
        qa, qb = DQ.Queue(samples[0], "BGRA", DQ.FULL, 8), DQ.Queue(samples[0], "BGRA", DQ.FULL, 8)
        d = RP.Delivery(qa, "BGRA", RP.RGBA_F32, True, 8); d.set()
        mark("planes begins"); assert DP.run_pass(qa, samples, count=5) == (5, [0] * 5); mark("planes ends")
        pa = DP.Delivery(qa, DP.PACKED, True, 8); pa.set()
        mark("packed a begins"); assert DP.run_pass(qa, samples, count=5) == (5, [0] * 5); mark("packed a ends")
        pb = DP.Delivery(qb, DP.PACKED, True, 8); pb.set()
        mark("packed b begins"); assert DP.run_pass(qb, samples, count=5) == (5, [0] * 5); mark("packed b ends")
        qa.close(); qb.close()
        planes = [RP.elements(p, RP.RGBA_F32, 65535) for p in RP.frame_planes("b64a", w, h)]
        packed = [RP.collected(f, "b64a", RP.RGBA_F32) for f in planes]
        src = RP.Source(planes, w, h, RP.RGBA_F32, True)
        row = RP.row_bytes("b64a", w)
        kind = RP.intra("b64a", "4444")
        with RP.Batch(kind, w, h, 4) as c, RP.Batch(kind, w, h, 4) as e:
            c.upload(packed[::-1], row)
            mark("call begins"); src.feed(c.L, c.b, 1, 2); mark("call ends")
            mark("pass c1 begins"); first = c.run(); mark("pass c1 ends")
            c.upload(packed, row)
            mark("pass c2 begins"); second = c.run(); mark("pass c2 ends")
            e.upload(packed, row)
            mark("pass d begins"); third = e.run(); mark("pass d ends")
            assert len(first) == 4 and len(second) == 4 and len(third) == 4
        with RP.chunked("3"), RP.Batch(kind, w, h, 4) as cut:
            mark("cut begins"); src.feed(cut.L, cut.b, 1, 3); mark("cut ends")
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
    assert names.count("k_dec_deliver_rgba") == 1 and names[-2:] == ["k_dec_blank", "k_dec_deliver_rgba"] and "k_dec_deliver" not in names, names
    assert planes[-1][1] == (24, 5, 1), planes[-1]                      # (dec_deliver_pieces(96 rows): four a piece; the pictures of the pass)
    assert [k for k, _ in packed_b][-2:] == ["k_dec_blank", "k_dec_deliver"] and "k_dec_deliver_rgba" not in [k for k, _ in packed_b], packed_b
    assert packed_a == packed_b and planes[:-1] == packed_b[:-1], (planes, packed_a, packed_b)
    call, c1, c2, d = launches("call"), launches("pass c1"), launches("pass c2"), launches("pass d")
    assert call == [("k_enc_collect_rgba", (24, 2, 1))], call           # (enc_collect_pieces(96 rows); frames)
    assert len(d) >= 4 and not [k for k, _ in d if k.startswith("k_enc_collect")], d
    assert c1 == d and c2 == d, (c1, c2, d)
    assert launches("cut") == [("k_enc_collect_rgba", (24, 2, 1)), ("k_enc_collect_rgba", (24, 1, 1))], launches("cut")      # (frames 1 - 2 of the first chunk, frame 3 of the second)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child()
