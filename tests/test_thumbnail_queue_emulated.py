"""tests/test_gpu_thumbnail_queue.py on the CPU against the emulated product library (cfhd_testlib.emulated_product: a device pointer is a host pointer; the kernels'
arithmetic host-compiled), and what only the CPU suite shows: the launch trace (HIPEMU_TRACE, in child processes) -- a thumbnail pass launches k_dec_ingest, k_dec_parse
and k_dec_thumbnail, one deliver kernel while a layout is set, one more inside wait per run of host-made pictures, and nothing of the decoder; an ordinary decode
batch beside it launches what it launches in a process that never made a thumbnail batch."""
import os, re, subprocess, sys
import pytest

if __name__ != "__main__":
    from cfhd_testlib import *
    import thumbnail_queue as TQ

    LAYOUT_IDS = [TQ.LAYOUT_NAMES[l] for l in TQ.LAYOUTS]


    @pytest.mark.parametrize("layout", TQ.LAYOUTS, ids=LAYOUT_IDS)
    @pytest.mark.parametrize("geometry", TQ.GEOMETRIES, ids=TQ.GEOMETRY_IDS)
    def test_emulated_every_picture_equals_cfhd_getthumbnail_on_every_way_out(geometry, layout):
        with emulated_product():
            TQ.check_exact(*geometry, layout)


    def test_emulated_a_picture_of_several_steps_a_workgroup_and_rows_longer_than_a_wave_step():
        """4224 x 96 (528 x 12 thumbnails), two samples, one layout: the emulated encoder needs a second or two a frame of this size."""
        with emulated_product():
            TQ.check_exact(*TQ.BIG, TQ.RGB10_F16, n=2)


    def test_emulated_the_geometry_of_a_display_height_that_is_no_multiple_of_8():
        with emulated_product():
            TQ.check_geometry_of_a_display_height_that_is_no_multiple_of_8()


    @pytest.mark.parametrize("case", [("422", 208, 104, TQ.PACKED, TQ.RGB10_F32), ("444", 176, 104, TQ.RGB10_U16, TQ.PACKED), ("422i", 192, 96, TQ.RGB10_F16, TQ.RGB10_U16)],
                             ids=["packed-then-f32", "u16-then-packed", "f16-then-u16"])
    def test_emulated_a_short_pass_touches_nothing_else_and_layouts_switch_between_passes(case):
        with emulated_product():
            TQ.check_short_pass_and_switching(*case)


    @pytest.mark.parametrize("layout", TQ.LAYOUTS, ids=LAYOUT_IDS)
    def test_emulated_failed_samples_get_cfhd_getthumbnails_status_and_zeros_among_intact_neighbours(layout):
        with emulated_product():
            TQ.check_failed_samples(layout, from_device=layout in (TQ.RGB10_U16, TQ.RGB10_F32))


    def test_emulated_gates():
        with emulated_product():
            TQ.check_gates()


    def test_emulated_kernel_names_and_times_follow_the_table():
        with emulated_product():
            TQ.check_kernel_names(times_positive=False)


    def test_emulated_one_pass_per_batch_several_batches_in_flight():
        with emulated_product():
            TQ.check_queue_rules()


def test_emulated_the_queue_refuses_under_host_entropy():
    env = dict(os.environ, CFHD_AMD_ENTROPY="host")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "host-entropy"], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "HOST ENTROPY REFUSED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def _mark(text): sys.stderr.write("[%s]\n" % text); sys.stderr.flush()


def _decode_pass(T, DQ, DP):
    """An ordinary YUY2 decode batch, one pass of 5, PACKED delivery: the same in both children."""
    plain = DQ.samples_of("422", 192, 96, "amd")
    q = DQ.Queue(plain[0], "YUY2", DQ.FULL, 8)
    d = DP.Delivery(q, DP.PACKED, True, 8); d.set()
    _mark("decode begins"); assert DP.run_pass(q, plain, count=5) == (5, [0] * 5); _mark("decode ends")
    q.close()


def _child(with_thumbnails):
    import cfhd_testlib as T
    import decode_queue as DQ
    import device_pictures as DP
    with T.emulated_product():
        if with_thumbnails:
            import thumbnail_queue as TQ
            samples = TQ.samples_of("422", 192, 96, src="amd")
            q = TQ.ThumbQueue(samples[0], 12)
            _mark("plain begins"); assert DP.run_pass(q, samples, count=5) == (5, [0] * 5); _mark("plain ends")
            d = TQ.Delivery(q, TQ.PACKED, True, 12); d.set()
            _mark("packed begins"); assert DP.run_pass(q, samples, count=5) == (5, [0] * 5); _mark("packed ends")
            d2 = TQ.Delivery(q, TQ.RGB10_F16, False, 12); d2.set()
            _mark("planes begins"); assert DP.run_pass(q, samples) == (8, [0] * 8); _mark("planes ends")
            failed, sizes = TQ.failed_pass()
            blob, offsets, _ = DQ.pack(failed)
            _mark("failed begins"); assert q.submit(blob, offsets, sizes) == 0; ret, status = q.wait(11); _mark("failed ends")
            assert ret == 5 and status[3] == 0 and status[7] == 0, (ret, status)
            q.close()
        _decode_pass(T, DQ, DP)
    print("TRACED")


def _trace(arg):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), arg], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "TRACED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stderr.splitlines()
    def launches(name):
        out = []
        for line in lines[lines.index("[%s begins]" % name) + 1: lines.index("[%s ends]" % name)]:
            m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)", line)
            if m: out.append((m.group(1).rsplit("::", 1)[-1], tuple(int(m.group(j)) for j in (3, 4, 5))))
        return out
    return launches


def test_a_thumbnail_pass_launches_three_kernels_and_a_deliver_and_nothing_of_the_decoder():
    launches = _trace("trace")
    FRONT = ["k_dec_ingest", "k_dec_parse", "k_dec_thumbnail"]
    plain, packed, planes, failed = launches("plain"), launches("packed"), launches("planes"), launches("failed")
    assert [k for k, _ in plain] == FRONT, plain
    assert plain[1][1] == (5, 1, 1) and plain[2][1] == (1, 5, 1), plain          # (a wave per sample; 288 pixels: one piece, the pictures of the pass)
    # dec_deliver_pieces(12 rows): four rows a piece
    assert [k for k, _ in packed] == FRONT + ["k_dec_deliver"] and packed[3][1] == (3, 5, 1), packed
    assert [k for k, _ in planes] == FRONT + ["k_dec_deliver_rgb10"] and planes[3][1] == (3, 8, 1), planes
    # the pass with failed samples: the launch of the pass over all eleven pictures, then, inside wait, one launch per run of host-made pictures: sample 3 (a size that
    # is no multiple of 4, which CFHD_GetThumbnail serves) and sample 7 (the RGB sample)
    assert [k for k, _ in failed] == FRONT + ["k_dec_deliver_rgb10"] * 3 and failed[3][1] == (3, 11, 1) and failed[4][1] == failed[5][1] == (3, 1, 1), failed
    for name in ("plain", "packed", "planes", "failed"):
        for k, _ in launches(name):
            assert k in FRONT + ["k_dec_deliver", "k_dec_deliver_rgb10"], (name, k)
            assert not (k.startswith("k_inv_") or k.startswith("k_half_") or k in ("k_dec_plan", "k_dec_index", "k_dec_tiles", "k_dec_lowpass", "k_dec_blank")), (name, k)
    # an ordinary decode batch in the same process launches exactly what one launches in a process that never made a thumbnail batch
    alone = _trace("trace-decode-only")("decode")
    beside = launches("decode")
    names = [k for k, _ in beside]
    assert "k_dec_blank" in names and names[-1] == "k_dec_deliver" and "k_dec_thumbnail" not in names and "k_dec_deliver_rgb10" not in names, names
    assert beside == alone, (beside, alone)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "host-entropy":
        import cfhd_testlib as T
        import thumbnail_queue as TQ
        with T.emulated_product():
            TQ.gates_under_host_entropy()
    else:
        _child(sys.argv[1] == "trace")
