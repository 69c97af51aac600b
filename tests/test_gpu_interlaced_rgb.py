"""Full-resolution RG48 / b64a / BGRA / BGRa decode of interlaced 4:2:2 samples through CFHD_DecodeSample: k_inv_frame_yuv422_rows16 (the inverse frame transform
into 16-bit rows, the reference's decoder.c:22027 TransformInverseFrameToRow16u) and k_yu64_to_rgb16 (its RGB conversion of those rows, bayer.c:13186; BGRA / BGRa in
the conversion's 8-bit mode).  Every decode equals tests/interlaced_rgb_model.py word for word / byte for byte -- the model is pinned on the reference decoder by
test_interlaced_rgb_model_vs_ref.py -- and the reference decoder runs beside it as a witness (RG48, b64a, BGRA: the reference's BGRa of an interlaced sample is not
its picture, see test_bgra_model_is_rg48_words_shifted_and_flipped)."""
import ctypes, os
import numpy as np
import pytest
from cfhd_testlib import *
from interlaced_rgb_model import model_decode

INTERLACED = 1
MATRIX_601 = 4
BADFORMAT = 3        # CFHD_ERROR_BADFORMAT


def _sample(w, h, flags):
    f, p = synth_yuy2(w, h, w + h)
    v = f.reshape(h, p)
    v[: h // 6, 0::2] = np.linspace(0, 255, w).astype(np.uint8)[None, :]
    v[h // 6: h // 3, 1::4] = 255; v[h // 6: h // 3, 3::4] = 0
    v[1::2] = np.roll(v[1::2], 8, axis=1)
    return ref_encode_frames([f], p, w, h, flags=flags | INTERLACED)[0]


def _view(buf, pitch, w, h, name):
    if name in ("BGRA", "BGRa"): return np.frombuffer(buf.tobytes(), np.uint8).reshape(-1, pitch)[:h, : w * 4]
    return np.frombuffer(buf.tobytes(), np.uint16).reshape(-1, pitch // 2)[:h, : w * (4 if name == "b64a" else 3)]


def _check(sample, w, h, name, color_space, decoder=None, witness=True):
    got, gpitch, aw, ah = amd_decode_sample(sample, fourcc(name), decoder=decoder)
    assert (aw, ah) == (w, h)
    mine = _view(got, gpitch, w, h, name)
    want = model_decode(sample, w, h, name, color_space)
    assert np.array_equal(mine, want), "%s: %d values differ from the model" % (name, (mine != want).sum())
    if witness and name != "BGRa":
        def leg():
            dec, dpitch = ref_decode_sample(sample, w, h, fourcc(name))
            img = _view(dec, dpitch, w, h, name)
            return np.array_equal(img, mine) or "%d values differ" % (img != mine).sum()
        reference_leg(leg, 4, "interlaced 4:2:2 -> %s" % name)
    return mine


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,name,flags", [(320, 240, "RG48", 0), (320, 240, "BGRa", 0), (336, 252, "b64a", MATRIX_601), (336, 252, "BGRA", 0),
                                            (720, 486, "BGRA", MATRIX_601), (720, 486, "RG48", MATRIX_601), (720, 486, "BGRa", 0), (1280, 720, "b64a", 0),
                                            (1280, 720, "BGRa", MATRIX_601), (1920, 1080, "RG48", 0), (1920, 1080, "BGRA", 0)])
def test_interlaced_rgb_decode_equals_model(w, h, name, flags):
    """709 and 601, a chroma band whose width is no multiple of 8 (336), a display height below the coded height (486), 720p and 1080i; both shapes of the
    frame kernel (CFHD_AMD_INVERSE=tile: the one-column fallback)."""
    sample = _sample(w, h, flags)
    cs = 1 if flags & MATRIX_601 else 2
    _check(sample, w, h, name, cs)
    os.environ["CFHD_AMD_INVERSE"] = "tile"
    try:
        _check(sample, w, h, name, cs, witness=False)
    finally:
        del os.environ["CFHD_AMD_INVERSE"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["RG48", "b64a", "BGRA", "BGRa"])
def test_interlaced_rgb_decode_of_1080i_qbist(name):
    frames, pitch = qbist_frames(10, 1)
    sample = ref_encode_frames(frames, pitch, 1920, 1080, flags=INTERLACED)[0]
    _check(sample, 1920, 1080, name, 2)


@pytest.mark.gpu
def test_interlaced_rgb_decode_of_peak_table_flicker_frames():
    """The difference band of a field-flicker frame carries a peak table; once with the GPU entropy decoder, once with the host one (CFHD_AMD_ENTROPY=host)."""
    w, h = 320, 64
    frames = [synth_yuy2(w, h, 3)[0], field_flicker_frame(w, h)[0]]
    samples = ref_encode_frames(frames, w * 2, w, h, PIX_YUY2, flags=INTERLACED)
    assert len(samples[1]) != len(samples[0])
    for name in ("RG48", "b64a", "BGRA", "BGRa"):
        for smp in samples: _check(smp, w, h, name, 2)
    os.environ["CFHD_AMD_ENTROPY"] = "host"
    try:
        for name in ("RG48", "BGRA"):
            for smp in samples: _check(smp, w, h, name, 2, witness=False)
    finally:
        del os.environ["CFHD_AMD_ENTROPY"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["BGRA", "RG48"])
def test_one_handle_alternates_interlaced_and_progressive(name):
    """One decoder handle: interlaced -> progressive -> interlaced.  BGRA takes another route on each (the 16-bit rows, then the fused k_inv_yuv422_rgb32)."""
    w, h = 320, 240
    inter = _sample(w, h, 0)
    f, p = synth_yuy2(w, h, 77)
    prog = ref_encode_frames([f], p, w, h)[0]
    L = product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        _check(inter, w, h, name, 2, decoder=dec, witness=False)
        got, gpitch, _, _ = amd_decode_sample(prog, fourcc(name), decoder=dec)
        plan = Plan(w, h, pixkind=PIXKIND[name], enc=ENC["422"])
        deq = oracle_decode_pyramid(prog, plan)
        want = oracle_inverse_rgb32_of_yuv422(plan, deq, True, 2)[:h] if name == "BGRA" else oracle_inverse_rgb16_of_yuv422(plan, deq, False, 2)[:h]
        assert np.array_equal(_view(got, gpitch, w, h, name), want)
        _check(inter, w, h, name, 2, decoder=dec, witness=False)
    finally:
        L.CFHD_CloseDecoder(dec)


@pytest.mark.gpu
def test_concurrent_interlaced_rgb_decoders_gather_and_stay_exact():
    """Four threads, each with its own handle, decode interlaced samples to RG48 and BGRA at the same time (two threads per format): overlapping calls are
    gathered into multi-frame launches (DecodeService, keyed on `interlaced`).  Every picture equals the model of its own sample."""
    import threading
    w, h = 640, 360
    samples = [_sample(w, h, 0), ref_encode_frames([field_flicker_frame(w, h)[0]], w * 2, w, h, flags=INTERLACED)[0]]
    want = {(name, k): model_decode(s, w, h, name, 2) for name in ("RG48", "BGRA") for k, s in enumerate(samples)}
    L = product()
    errors = []

    def worker(t):
        try:
            name = ("RG48", "BGRA")[t % 2]
            dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
            aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
            first = ctypes.create_string_buffer(samples[0], len(samples[0]))
            assert L.CFHD_PrepareToDecode(dec, 0, 0, fourcc(name), 1, 0, first, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
            p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
            out = np.zeros(p.value * h, np.uint8)
            for r in range(10):
                k = (t + r) % 2
                sb = ctypes.create_string_buffer(samples[k], len(samples[k]))
                out[:] = 7
                rc = L.CFHD_DecodeSample(dec, sb, len(samples[k]), out.ctypes.data_as(ctypes.c_void_p), p.value)
                assert rc == 0, (rc, t, r, amd_last_error())
                assert np.array_equal(_view(out, p.value, w, h, name), want[(name, k)]), "thread %d round %d" % (t, r)
            L.CFHD_CloseDecoder(dec)
        except BaseException as e:                                 # noqa: surfaced in the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads: t.start()
    for t in threads: t.join()
    if errors: raise errors[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["YU64", "v210", "RG24", "r210", "DPX0", "AB10", "AR10"])
def test_remaining_interlaced_full_resolution_gates(name):
    """What stays refused for interlaced samples at full resolution: YU64, v210, RG24 and the 10-bit RGB words -- BADFORMAT, at CFHD_PrepareToDecode or with a
    zeroed picture at CFHD_DecodeSample."""
    w, h = 384, 96
    sample = _sample(w, h, 0)
    L = product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
        sb = ctypes.create_string_buffer(sample, len(sample))
        rc = L.CFHD_PrepareToDecode(dec, 0, 0, fourcc(name), 1, 0, sb, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af))
        if rc != 0:
            assert rc == BADFORMAT
            return
        p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
        out = np.ones(p.value * ah.value, np.uint8)
        assert L.CFHD_DecodeSample(dec, sb, len(sample), out.ctypes.data_as(ctypes.c_void_p), p.value) == BADFORMAT
        assert not out.any()
    finally:
        L.CFHD_CloseDecoder(dec)
