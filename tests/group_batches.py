"""Batches of two-frame groups on the frame queue (cfhd_amd_batch_create_ex with CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP): the helpers and test bodies shared by
tests/test_gpu_group_batches.py (hardware) and tests/test_group_batches_emulated.py (the same functions inside cfhd_testlib.emulated_product()).

What is checked against what:
  samples   one CFHD_EncodeSample handle fed the same frames over two passes (+ one call that flushes the last P-frame sample), CFHD_AMD_ENTROPY=device so that the
            handle fails rather than hand a group to the host writer; byte for byte after mask_volatile_metadata.  One live-reference witness per input.
  pictures  16-bit outputs: CFHD_DecodeSample's pictures of the same samples, word for word (pinned on the reference by tests/test_gpu_group_outputs.py);
            8-bit 4:2:2: the oracle's group inverse with dither 0 or 1, byte by byte, and the PSNR bar of tests/test_gpu_gop.py.
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *

GOP = ENCODING_FLAGS_2FRAME_GOP
INTERLACED = 1
MATRIX_601 = 4
FOURCCS = {"YUY2": PIX_YUY2, "2vuy": PIX_2VUY, "v210": PIX_V210, "RG48": PIX_RG48, "b64a": PIX_B64A, "YU64": PIX_YU64, "RG64": fourcc("RG64"), "a214": fourcc("a214"),
           "RG24": PIX_RG24, "BGRA": PIX_BGRA, "BGRa": PIX_BGRa}
# (w, h, input, interlaced, nframes): odd chroma lowpass widths and a display height that is no multiple of 8 (336 x 252), whole 48-pixel groups of v210 (384), the
# colour conversion in the loader (RG48), an input without a decoder output (RG64, a214), peak tables (interlaced flicker), 35 groups (past kLowLatencyFrames)
SAMPLE_CASES = [(320, 240, "YUY2", 0, 4), (336, 252, "2vuy", 0, 6), (384, 96, "v210", 0, 4), (320, 240, "RG48", 0, 4), (320, 240, "RG64", 0, 2), (320, 240, "a214", 0, 4),
                (336, 252, "YUY2", 1, 4), (192, 96, "YUY2", 0, 70)]
ROUNDTRIP_INPUTS = ("YUY2", "2vuy", "YU64", "v210", "RG48", "b64a")
# (w, h, input, interlaced, nframes, extra encoding flags): the sample cases that have an output, YU64 and b64a, and RG48 tagged 601 (frame 1 of every group still converts with 709)
PICTURE_CASES = [c + (0,) for c in SAMPLE_CASES if c[2] in ROUNDTRIP_INPUTS] + [(320, 240, "YU64", 0, 2, 0), (320, 240, "b64a", 0, 4, 0), (320, 240, "RG48", 0, 4, MATRIX_601)]


def lib():
    L = product()
    if not getattr(L, "_group_batches_declared", False):
        V = ctypes.c_void_p
        L.cfhd_amd_batch_create_ex.restype = V
        L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32] + [ctypes.c_int] * 4
        L.cfhd_amd_batch_destroy.argtypes = [V]; L.cfhd_amd_batch_destroy.restype = None
        L.cfhd_amd_batch_upload.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        for f in (L.cfhd_amd_batch_roundtrip, L.cfhd_amd_batch_wait): f.restype = ctypes.c_longlong; f.argtypes = [V]
        L.cfhd_amd_batch_submit.argtypes = [V]
        L.cfhd_amd_batch_submit_host.argtypes = [V, V, ctypes.c_size_t, ctypes.c_int, V, ctypes.c_size_t, ctypes.c_int]
        L.cfhd_amd_batch_get_sample.argtypes = [V, ctypes.c_int, ctypes.POINTER(V), ctypes.POINTER(ctypes.c_size_t)]
        L.cfhd_amd_batch_download_output.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
        L.cfhd_amd_batch_kernel_ms.restype = ctypes.c_float; L.cfhd_amd_batch_kernel_ms.argtypes = [V, ctypes.c_int]
        L.cfhd_amd_batch_kernel_name.restype = ctypes.c_char_p; L.cfhd_amd_batch_kernel_name.argtypes = [V, ctypes.c_int]
        L.cfhd_amd_batch_dx_stats.argtypes = [V, V]
        L.cfhd_amd_set_clip_guid.argtypes = [ctypes.c_char_p]; L.cfhd_amd_set_clip_guid.restype = None
        L._group_batches_declared = True
    return L


def sequence_header(L, b):
    """(rc, bytes) of cfhd_amd_batch_get_sequence_header; a library without the entry point fails the test that asks."""
    fn = L.cfhd_amd_batch_get_sequence_header
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    p = ctypes.c_void_p(); n = ctypes.c_size_t()
    rc = fn(b, ctypes.byref(p), ctypes.byref(n))
    return rc, (ctypes.string_at(p, n.value) if rc == 0 else b"")


_frames = {}


def _flat_bottom_frame(w, h, i):
    """Frame i of a slowly moving YUY2 sequence whose rows below 2/3 of the height repeat.  Why: the unprescaled wavelets of a group inherit the defect of the
    reference's last inverse row (InvPlaneJob::ll_bottom_row_high; CFHD_AMD_GOP_BOTTOM_ROWS=fixed is +5 dB), whose error grows with the picture's vertical gradient at
    its bottom edge.  On 96 rows that edge is a large share of the picture: the pictures of synth_yuy2 come back at 36.5 .. 39.8 dB by the phase of the frame --
    byte for byte inside the oracle's interval, i.e. the reference's decoder gives the same --, these at 48.8 .. 49.0 dB.  The 38 dB bar is about the decoder, not
    about that edge, so the 35-group case takes pictures without a gradient there."""
    rng = np.random.default_rng(700 + i)
    y, x = np.mgrid[0:h, 0:w]
    y = np.minimum(y, 2 * h // 3)
    luma = 128 + 90 * np.sin(x / 37.0 + i / 8.0) * np.cos(y / 23.0) + rng.normal(0, 1, (h, w))
    cb = 128 + 60 * np.sin(x / 91.0 + i / 8.0) + rng.normal(0, 1, (h, w))
    cr = 128 + 60 * np.cos(y / 67.0) + rng.normal(0, 1, (h, w))
    f = np.zeros((h, w * 2), np.uint8)
    f[:, 0::2] = np.clip(luma, 0, 255).astype(np.uint8); f[:, 1::4] = np.clip(cb[:, 0::2], 0, 255).astype(np.uint8); f[:, 3::4] = np.clip(cr[:, 0::2], 0, 255).astype(np.uint8)
    return f.reshape(-1)


def case_frames(w, h, name, interlaced, nframes):
    """nframes distinct frames of the input (computed once, shared, read-only) and their pitch."""
    key = (w, h, name, interlaced, nframes)
    if key not in _frames:
        import test_gop, gop_input_frames, avid_frames
        if name == "YUY2" and not interlaced and h < 240:
            fr, pitch = [_flat_bottom_frame(w, h, i) for i in range(nframes)], w * 2
        elif name in ("YUY2", "2vuy"):
            fr = test_gop._interlaced_frames(w, h, nframes, FOURCCS[name], True) if interlaced else test_gop._frames(w, h, nframes, FOURCCS[name])
            fr, pitch = [np.ascontiguousarray(f) for f in fr], w * 2
        elif name == "a214": fr, pitch, _ = avid_frames.frames(name, w, h, nframes)
        else: fr, pitch = gop_input_frames.frames(name, w, h, nframes)
        _frames[key] = (list(fr), pitch)
    return _frames[key]


def picture_pitch(name, w):
    return {"YUY2": 2 * w, "2vuy": 2 * w, "YU64": 4 * w, "RG48": 6 * w, "b64a": 8 * w, "v210": (w + 47) // 48 * 128}[name]


class Batch:
    """One batch of two-frame groups with its frames in HBM."""
    def __init__(self, w, h, name, interlaced, nframes, mode, flags=0, quality=QUALITY_FILMSCAN1, frames=None):
        self.L = lib(); self.w, self.h, self.name, self.n, self.mode = w, h, name, nframes, mode
        self.b = self.L.cfhd_amd_batch_create_ex(w, h, FOURCCS[name], ENCODED_YUV422, GOP | (INTERLACED if interlaced else 0) | flags, quality, nframes, 1, mode)
        assert self.b, "cfhd_amd_batch_create_ex -> NULL (%s)" % amd_last_error()
        self.frames, self.pitch = frames if frames is not None else case_frames(w, h, name, interlaced, nframes)
        for i, f in enumerate(self.frames):
            assert self.L.cfhd_amd_batch_upload(self.b, i, np.asarray(f).ctypes.data_as(ctypes.c_void_p), self.pitch) == 0, amd_last_error()

    def samples(self):
        out = []
        for i in range(self.n):
            p = ctypes.c_void_p(); n = ctypes.c_size_t()
            assert self.L.cfhd_amd_batch_get_sample(self.b, i, ctypes.byref(p), ctypes.byref(n)) == 0
            out.append(ctypes.string_at(p, n.value))
        return out

    def pictures(self):
        pitch = picture_pitch(self.name, self.w); out = []
        for i in range(self.n):
            o = np.full(pitch * self.h, 7, np.uint8)
            assert self.L.cfhd_amd_batch_download_output(self.b, i, o.ctypes.data_as(ctypes.c_void_p), pitch) == 0, amd_last_error()
            out.append(o)
        return out

    def roundtrip(self):
        total = self.L.cfhd_amd_batch_roundtrip(self.b)
        assert total > 0, "pass -> %d (%s)" % (total, amd_last_error())
        return total

    def close(self):
        if self.b: self.L.cfhd_amd_batch_destroy(self.b); self.b = None


class device_entropy:
    """CFHD_AMD_ENTROPY=device: a group the C ABI's handle would hand to the host writer fails the call instead."""
    def __enter__(self): self.old = os.environ.get("CFHD_AMD_ENTROPY"); os.environ["CFHD_AMD_ENTROPY"] = "device"
    def __exit__(self, *a):
        if self.old is None: os.environ.pop("CFHD_AMD_ENTROPY", None)
        else: os.environ["CFHD_AMD_ENTROPY"] = self.old


_witnessed = set()


def check_samples_equal_the_c_abi_stream(w, h, name, interlaced, nframes):
    frames, pitch = case_frames(w, h, name, interlaced, nframes)
    flags = GOP | (INTERLACED if interlaced else 0)
    fed = list(frames) + list(frames) + [frames[0]]
    with device_entropy():
        stream = amd_encode_frames(fed, pitch, w, h, FOURCCS[name], flags=flags)
        mode = 0 if name in ROUNDTRIP_INPUTS else 1
        bt = Batch(w, h, name, interlaced, nframes, mode)
        try:
            rc, header = sequence_header(bt.L, bt.b)
            assert rc == 0 and len(header) == 40 and header == stream[0], "sequence header"
            mine = [header]
            for k in range(2):
                total = bt.roundtrip()
                s = bt.samples()
                assert total == sum(len(x) for x in s[0::2])
                assert all(len(x) == 24 for x in s[1::2])
                mine += s
        finally:
            bt.close()
    assert [len(s) for s in mine] == [len(s) for s in stream]
    for i, (a, b) in enumerate(zip(mine, stream)):
        assert mask_volatile_metadata(a) == mask_volatile_metadata(b), "sample %d of the batch differs from the handle's stream" % i
    if name in _witnessed or not have_ref(): return
    _witnessed.add(name)
    def leg():
        refs = ref_encode_frames(fed, pitch, w, h, pixfmt=FOURCCS[name], flags=flags)
        if [len(s) for s in refs] != [len(s) for s in mine]: return "sizes differ"
        for i, (a, b) in enumerate(zip(mine, refs)):
            if mask_volatile_metadata(a) != mask_volatile_metadata(b): return "sample %d differs from the reference" % i
        return True
    reference_leg(leg, 2, "group batches: samples from %s" % name)


def cabi_group_pictures(samples, name):
    """CFHD_DecodeSample's pictures of [group, P-frame sample, group, ...] through one handle prepared on the first group."""
    L = product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    try:
        aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
        sb = ctypes.create_string_buffer(samples[0], len(samples[0]))
        assert L.CFHD_PrepareToDecode(dec, 0, 0, FOURCCS[name], 1, 0, sb, 512, ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
        p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
        outs = []
        for s in samples:
            sb = ctypes.create_string_buffer(s, len(s)); out = np.full(p.value * ah.value, 7, np.uint8)
            assert L.CFHD_DecodeSample(dec, sb, len(s), out.ctypes.data_as(ctypes.c_void_p), p.value) == 0, amd_last_error()
            outs.append(out)
        return outs, aw.value, ah.value, p.value
    finally:
        L.CFHD_CloseDecoder(dec)


def check_pictures(w, h, name, interlaced, nframes, flags):
    bt = Batch(w, h, name, interlaced, nframes, 0, flags)
    try:
        bt.roundtrip()
        samples, pictures = bt.samples(), bt.pictures()
    finally:
        bt.close()
    pitch = picture_pitch(name, w)
    if name in ("YUY2", "2vuy"):
        # the acceptance of tests/test_gpu_gop.py: every byte the oracle's group inverse with dither 0 or with dither 1; progressive groups: the PSNR bar too
        gp = GopPlan(w, h, pixkind=PIXKIND[name], interlaced=int(bool(interlaced)))
        for g in range(nframes // 2):
            co = oracle_decode_group(samples[2 * g], gp)
            lo = oracle_inverse_gop(gp, co, 0, uyvy=int(name == "2vuy")); hi = oracle_inverse_gop(gp, co, 1, uyvy=int(name == "2vuy"))
            for f in range(2):
                img = pictures[2 * g + f].reshape(h, pitch)
                ok = (img == lo[f][:h]) | (img == hi[f][:h])
                assert ok.all(), "group %d frame %d: %d bytes outside the dither interval" % (g, f, (~ok).sum())
                if not interlaced: assert psnr_yuy2(img, np.asarray(bt.frames[2 * g + f]).reshape(h, pitch)) > 38.0
        return
    with device_entropy():
        want, aw, ah, wpitch = cabi_group_pictures(samples, name)
    assert (aw, ah, wpitch) == (w, h, pitch)
    for i in range(nframes):
        a, b = pictures[i].view(np.uint16), want[i].view(np.uint16)
        assert np.array_equal(a, b), "frame %d: %d words differ from CFHD_DecodeSample's picture" % (i, (a != b).sum())


def check_queue():
    """Two batches in flight through submit / wait and one through submit_host with its pictures: the same samples and pictures as synchronous passes with the same
    step numbers; between submit and wait every other entry point refuses the batch."""
    L = lib()
    L.cfhd_amd_set_clip_guid(bytes(range(16)))
    w, h, name, n = 320, 240, "YUY2", 4
    frames, pitch = case_frames(w, h, name, 0, 2 * n)
    sets = [(frames[:n], pitch), (frames[n:], pitch)]
    def synchronous(fs, passes):
        bt = Batch(w, h, name, 0, n, 0, frames=fs)
        try:
            out = []
            for _ in range(passes): bt.roundtrip(); out.append((bt.samples(), bt.pictures()))
            return out
        finally:
            bt.close()
    want = [synchronous(fs, 2) for fs in sets]
    queued = [Batch(w, h, name, 0, n, 0, frames=fs) for fs in sets]
    try:
        for step in range(2):
            for bt in queued: assert L.cfhd_amd_batch_submit(bt.b) == 0
            bt = queued[0]
            p = ctypes.c_void_p(); sz = ctypes.c_size_t(); buf = np.zeros(pitch * h, np.uint8); stats = (ctypes.c_uint32 * 16)()
            assert L.cfhd_amd_batch_roundtrip(bt.b) == -1 and L.cfhd_amd_batch_submit(bt.b) == -1
            assert L.cfhd_amd_batch_submit_host(bt.b, buf.ctypes.data_as(ctypes.c_void_p), 0, pitch, None, 0, 0) == -1
            assert L.cfhd_amd_batch_upload(bt.b, 0, buf.ctypes.data_as(ctypes.c_void_p), pitch) == -1
            assert L.cfhd_amd_batch_get_sample(bt.b, 0, ctypes.byref(p), ctypes.byref(sz)) == -1
            assert sequence_header(L, bt.b)[0] == -1
            assert L.cfhd_amd_batch_download_output(bt.b, 0, buf.ctypes.data_as(ctypes.c_void_p), pitch) == -1
            assert L.cfhd_amd_batch_kernel_ms(bt.b, 0) == 0 and L.cfhd_amd_batch_kernel_name(bt.b, 0) == b"" and L.cfhd_amd_batch_dx_stats(bt.b, stats) == -1
            for k, bt in enumerate(queued):
                total = L.cfhd_amd_batch_wait(bt.b)
                s, pics = bt.samples(), bt.pictures()
                assert total == sum(len(x) for x in s[0::2])
                assert [mask_volatile_metadata(x) for x in s] == [mask_volatile_metadata(x) for x in want[k][step][0]], "batch %d step %d: samples" % (k, step)
                assert all(np.array_equal(a, b) for a, b in zip(pics, want[k][step][1])), "batch %d step %d: pictures" % (k, step)
            assert L.cfhd_amd_batch_wait(queued[0].b) == -1          # nothing in flight
    finally:
        for bt in queued: bt.close()
    # fed from host memory, pictures coming back: frames at their own stride with a gap between them
    fs = sets[0][0]
    stride = pitch * h + 256
    src = np.zeros(stride * n, np.uint8); dst = np.full(stride * n, 9, np.uint8)
    for i, f in enumerate(fs): src[i * stride: i * stride + pitch * h] = np.asarray(f)
    L.cfhd_amd_batch_create_ex.restype = ctypes.c_void_p
    b = L.cfhd_amd_batch_create_ex(w, h, FOURCCS[name], ENCODED_YUV422, GOP, QUALITY_FILMSCAN1, n, 1, 0)
    assert b
    try:
        for step in range(2):
            assert L.cfhd_amd_batch_submit_host(b, src.ctypes.data_as(ctypes.c_void_p), stride, pitch, dst.ctypes.data_as(ctypes.c_void_p), stride, pitch) == 0, amd_last_error()
            total = L.cfhd_amd_batch_wait(b)
            assert total == sum(len(x) for x in want[0][step][0][0::2]), total
            for i in range(n):
                assert np.array_equal(dst[i * stride: i * stride + pitch * h], want[0][step][1][i]), "host-fed step %d picture %d" % (step, i)
                assert (dst[i * stride + pitch * h: (i + 1) * stride] == 9).all()
            p = ctypes.c_void_p(); sz = ctypes.c_size_t()
            for i in range(n):
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                assert mask_volatile_metadata(ctypes.string_at(p, sz.value)) == mask_volatile_metadata(want[0][step][0][i]), "host-fed step %d sample %d" % (step, i)
    finally:
        L.cfhd_amd_batch_destroy(b)


def check_gates():
    L = lib()
    create = lambda w, h, name, enc, flags, quality, n, mode: L.cfhd_amd_batch_create_ex(w, h, FOURCCS[name], enc, flags, quality, n, 1, mode)
    def refused(*a):
        b = create(*a)
        if b: L.cfhd_amd_batch_destroy(b)
        return not b
    for mode in (0, 1):
        assert refused(320, 240, "YUY2", ENCODED_YUV422, GOP, QUALITY_FILMSCAN1, 3, mode), "odd frame count"
        assert refused(320, 240, "YUY2", ENCODED_YUV422, GOP, 5, 4, mode), "FILMSCAN2: the group tables follow the previous key sample"
        for name in ("RG24", "BGRA", "BGRa"): assert refused(320, 240, name, ENCODED_YUV422, GOP, QUALITY_FILMSCAN1, 4, mode), name
        assert refused(320, 240, "RG48", ENCODED_RGB444, GOP, QUALITY_FILMSCAN1, 4, mode), "4:4:4 with the group flag"
        assert refused(200, 240, "YUY2", ENCODED_YUV422, GOP, QUALITY_FILMSCAN1, 4, mode), "width 200"
    for name in ("RG64", "a214"): assert refused(320, 240, name, ENCODED_YUV422, GOP, QUALITY_FILMSCAN1, 4, 0), name + " has no decoder output"
    assert refused(320, 240, "v210", ENCODED_YUV422, GOP | INTERLACED, QUALITY_FILMSCAN1, 4, 1), "interlaced groups: YUY2 / 2vuy"
    old = os.environ.get("CFHD_AMD_ENTROPY")
    os.environ["CFHD_AMD_ENTROPY"] = "host"
    try:
        assert refused(320, 240, "YUY2", ENCODED_YUV422, GOP, QUALITY_FILMSCAN1, 4, 0), "host entropy"
    finally:
        if old is None: os.environ.pop("CFHD_AMD_ENTROPY")
        else: os.environ["CFHD_AMD_ENTROPY"] = old
    # a batch without the flag still writes intra samples, and has no sequence header
    w, h = 320, 240
    frames, pitch = case_frames(w, h, "YUY2", 0, 4)
    b = create(w, h, "YUY2", ENCODED_YUV422, 0, QUALITY_FILMSCAN1, 2, 1)
    assert b
    try:
        for i in range(2): assert L.cfhd_amd_batch_upload(b, i, np.asarray(frames[i]).ctypes.data_as(ctypes.c_void_p), pitch) == 0
        assert L.cfhd_amd_batch_roundtrip(b) > 0
        p = ctypes.c_void_p(); sz = ctypes.c_size_t()
        assert L.cfhd_amd_batch_get_sample(b, 1, ctypes.byref(p), ctypes.byref(sz)) == 0
        intra = amd_encode_frames(frames[:2], pitch, w, h)
        assert mask_volatile_metadata(ctypes.string_at(p, sz.value)) == mask_volatile_metadata(intra[1])
        assert sequence_header(L, b)[0] == -1
    finally:
        L.cfhd_amd_batch_destroy(b)
