"""The five Avid 4:2:2 encoder inputs (avu8, av16, a106, a214, av28), CPU side: the emulated product library (tests/hipemu: the C ABI, the job tables and the
loaders of k_fwd_packed16 / k_fwd_gop_packed16 from the unmodified kernel source) against the compiled reference encoder, byte for byte -- intra samples, and the
sequence header, group samples and P-frame headers of two-frame groups -- plus the refusals and the launch routes.

The reference encodes all five and its own decoder takes every sample as YU64 (probed at 192 x 96, FILMSCAN1), so all five are served.  The frames
(tests/avid_frames.py) carry what a wrong unpack would trip over: 0 and 255 (avu8), random low six bits (av16 / a106), the whole int16 range with the values where
C's division and an arithmetic shift part (a214), every two-bit value in every position of the upper plane (av28).

tests/golden/avid_input_routes.json (`python tests/test_avid_inputs_emulated.py record`) holds, per layout, what one encode-only batch of two frames and one group
encoder launch on the emulator -- recorded from this library, not from the reference: which kernels, over which grids, and a digest of the samples."""
import ctypes, hashlib, json, os, re, subprocess, sys
import numpy as np
import pytest
import cfhd_testlib as T
import avid_frames as A

GOP, INTERLACED = T.ENCODING_FLAGS_2FRAME_GOP, 1
QUALITY_LOW, QUALITY_FILMSCAN2 = 1, 5       # Common/CFHDTypes.h:203-207
BADFORMAT = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avid_input_routes.json")
W, H = 192, 96


def _same_samples(name, w, h, n, flags=0, quality=T.QUALITY_FILMSCAN1, data=None, pitch=None):
    """The product's samples of n frames, after they have been found equal to the live reference encoder's."""
    assert T.have_ref(), "oracle/_ref/libcfhd_ref.so is missing"
    if data is None: data, pitch, _ = A.frames(name, w, h, n)
    with T.emulated_product():
        mine = T.amd_encode_frames(data, pitch, w, h, A.FOURCC[name], flags=flags, quality=quality)
    refs = T.ref_encode_frames(data, pitch, w, h, pixfmt=A.FOURCC[name], flags=flags, quality=quality)
    assert [len(s) for s in mine] == [len(s) for s in refs]
    for i, (a, b) in enumerate(zip(mine, refs)):
        assert T.mask_volatile_metadata(a) == T.mask_volatile_metadata(b), "sample %d differs from the reference" % i
    return mine


def test_the_a214_frame_holds_the_values_where_division_and_shift_part():
    data, _, _ = A.frames("a214", W, H, 1)
    words = A.words_of("a214", data[0], W, H)
    assert A.shift_and_division_differ(words) >= 1000
    for v in (-1, -16383, 16384, -32768, 32767): assert (words[:, 1::2] == v).any() and (words[:, 0::2] == v).any(), v      # luma and chroma
    assert (words[:, 0::2].astype(int) < -8192).sum() > 100 and (words[:, 0::2].astype(int) > 8191).sum() > 100
    up = np.asarray(A.frames("av28", W, H, 1)[0][0])[: W * H // 2]
    for pos in range(4): assert set(np.unique((up >> (2 * pos)) & 3)) == {0, 1, 2, 3}
    b = np.asarray(A.frames("avu8", W, H, 1)[0][0])
    assert b.min() == 0 and b.max() == 255
    assert len(np.unique(np.asarray(A.frames("av16", W, H, 1)[0][0]).view(np.uint16) & 63)) == 64


# 192 x 96: three tile rows of one luma tile; 208 x 104: a width that is a multiple of 16 and not of 64 -- a second luma tile of 8 of 64 columns, 4 in the chroma planes
@pytest.mark.parametrize("quality", [T.QUALITY_FILMSCAN1, QUALITY_LOW])
@pytest.mark.parametrize("w,h", [(192, 96), (208, 104)])
@pytest.mark.parametrize("name", A.LAYOUTS)
def test_intra_samples_equal_the_reference(name, w, h, quality):
    mine = _same_samples(name, w, h, 2, quality=quality)
    assert mine[0] != mine[1] and min(len(s) for s in mine) > 4096
    assert mine[0][35] == A.COLOR_FORMAT[name]          # the input format tuple of the sample header


@pytest.mark.parametrize("name", A.LAYOUTS)
def test_group_stream_equals_the_reference(name):
    mine = _same_samples(name, W, H, 4, flags=GOP, quality=QUALITY_FILMSCAN2)
    assert len(mine[0]) == 40 and len(mine[2]) == 24 and min(len(mine[1]), len(mine[3])) > 4096      # sequence header, group, P-frame header, group
    assert mine[1] != mine[3]


def test_negative_pitch_a106():
    """The rows in memory order from the last row's address (Codec/encoder.c:1957), as tests/test_gop_inputs.py::test_negative_pitch shows for YU64."""
    data, pitch, _ = A.frames("a106", W, H, 4)
    for flags in (0, GOP):
        mine = _same_samples("a106", W, H, 4, flags=flags, data=A.from_last_row(data, pitch, H), pitch=-pitch)
        with T.emulated_product():
            forward = T.amd_encode_frames(data, pitch, W, H, A.FOURCC["a106"], flags=flags)
        assert [T.mask_volatile_metadata(s) for s in mine] == [T.mask_volatile_metadata(s) for s in forward]


def test_av28_ignores_the_pitch():
    """Both planes are walked as tightly packed rows whatever pitch the caller names (Codec/frame.c:13179-13186): the reference and the product alike."""
    data, pitch, _ = A.frames("av28", W, H, 2)
    for flags in (0, GOP):
        plain = _same_samples("av28", W, H, 2, flags=flags)
        odd = _same_samples("av28", W, H, 2, flags=flags, data=data, pitch=5 * W + 64)
        assert [T.mask_volatile_metadata(s) for s in odd] == [T.mask_volatile_metadata(s) for s in plain]


def test_refusals():
    """The five with CFHD_ENCODING_FLAGS_YUV_INTERLACED, towards any encoded format but 4:2:2, at widths that are no multiples of 16: BADFORMAT at
    CFHD_PrepareToEncode.  A batch that would decode back (mode 0) is not created: there is no decoder output of these layouts."""
    with T.emulated_product() as L:
        L.cfhd_amd_batch_create_ex.restype = ctypes.c_void_p
        L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.cfhd_amd_batch_destroy.argtypes = [ctypes.c_void_p]
        enc = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
        prep = lambda name, encoded, flags, w=W: L.CFHD_PrepareToEncode(enc, w, H, A.FOURCC[name], encoded, flags, T.QUALITY_FILMSCAN1)
        for name in A.LAYOUTS:
            assert prep(name, T.ENCODED_YUV422, 0) == 0 and prep(name, T.ENCODED_YUV422, GOP) == 0, name
            assert prep(name, T.ENCODED_YUV422, INTERLACED) == BADFORMAT and prep(name, T.ENCODED_YUV422, GOP | INTERLACED) == BADFORMAT, name
            for encoded in (T.ENCODED_RGB444, T.ENCODED_RGBA4444, T.ENCODED_BAYER): assert prep(name, encoded, 0) == BADFORMAT, (name, encoded)
            assert prep(name, T.ENCODED_YUV422, 0, 200) == BADFORMAT and prep(name, T.ENCODED_YUV422, GOP, 200) == BADFORMAT, name      # width % 16
            assert not L.cfhd_amd_batch_create_ex(W, H, A.FOURCC[name], T.ENCODED_YUV422, 0, T.QUALITY_FILMSCAN1, 2, 1, 0), name
            b = L.cfhd_amd_batch_create_ex(W, H, A.FOURCC[name], T.ENCODED_YUV422, 0, T.QUALITY_FILMSCAN1, 2, 1, 1)
            assert b, name
            L.cfhd_amd_batch_destroy(b)
        L.CFHD_CloseEncoder(enc)


def test_the_input_format_list_keeps_its_entries():
    """CFHD_GetInputFormats does not advertise the Avid codes, as the reference's own list does not (EncoderSDK/SampleEncoder.cpp:71-88)."""
    with T.emulated_product() as L:
        enc = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
        arr = (ctypes.c_uint32 * 64)(); n = ctypes.c_int()
        assert L.CFHD_GetInputFormats(enc, arr, 64, ctypes.byref(n)) == 0
        L.CFHD_CloseEncoder(enc)
    assert not set(arr[: n.value]) & set(A.FOURCC.values())


# ---- launch routes: a fresh child per case (HIPEMU_TRACE is read once per process), the emulator's launch trace as the witness
CASES = {}
for _name in A.LAYOUTS:
    CASES["422 " + _name] = (_name, 0)
    CASES["gop " + _name] = (_name, GOP)
FRAMES = 2
FORWARD = re.compile(r"k_fwd_|k_unpack_byr4$|k_gop_")


def _child(case):
    """'RESULT <json>' ([return codes, reported level-1 kernel, digest of the samples]) on stdout, the trace on stderr: an encode-only batch of two frames, or two
    CFHD_EncodeSample calls of a group encoder."""
    name, flags = CASES[case]
    data, pitch, _ = A.frames(name, W, H, FRAMES)
    digest, rcs = hashlib.sha256(), []
    with T.emulated_product() as L:
        if flags & GOP:
            L.cfhd_amd_encoder_kernel_name.restype = ctypes.c_char_p
            L.cfhd_amd_encoder_kernel_name.argtypes = [ctypes.c_void_p]
            enc = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
            rcs.append(L.CFHD_PrepareToEncode(enc, W, H, A.FOURCC[name], T.ENCODED_YUV422, flags, T.QUALITY_FILMSCAN1))
            reported = L.cfhd_amd_encoder_kernel_name(enc).decode()
            for f in data if rcs[0] == 0 else []:
                rcs.append(L.CFHD_EncodeSample(enc, f.ctypes.data_as(ctypes.c_void_p), pitch))
                if rcs[-1]: break
                p = ctypes.c_void_p(); n = ctypes.c_size_t()
                assert L.CFHD_GetSampleData(enc, ctypes.byref(p), ctypes.byref(n)) == 0
                digest.update(T.mask_volatile_metadata(ctypes.string_at(p, n.value)))
            L.CFHD_CloseEncoder(enc)
        else:
            L.cfhd_amd_batch_create_ex.restype = ctypes.c_void_p
            L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
            L.cfhd_amd_batch_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
            L.cfhd_amd_batch_roundtrip.restype = ctypes.c_longlong
            L.cfhd_amd_batch_roundtrip.argtypes = [ctypes.c_void_p]
            L.cfhd_amd_batch_kernel_name.restype = ctypes.c_char_p
            L.cfhd_amd_batch_kernel_name.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.cfhd_amd_batch_get_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
            L.cfhd_amd_batch_destroy.argtypes = [ctypes.c_void_p]
            b = L.cfhd_amd_batch_create_ex(W, H, A.FOURCC[name], T.ENCODED_YUV422, flags, T.QUALITY_FILMSCAN1, FRAMES, 1, 1)      # (mode 1: encode only)
            assert b, T.amd_last_error()
            for i, f in enumerate(data): assert L.cfhd_amd_batch_upload(b, i, f.ctypes.data_as(ctypes.c_void_p), pitch) == 0
            reported = L.cfhd_amd_batch_kernel_name(b, 0).decode()
            rc = L.cfhd_amd_batch_roundtrip(b)
            rcs.append(rc if rc < 0 else 0)
            for i in range(FRAMES if rc > 0 else 0):
                p = ctypes.c_void_p(); sz = ctypes.c_size_t()
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                digest.update(T.mask_volatile_metadata(ctypes.string_at(p, sz.value)))
            L.cfhd_amd_batch_destroy(b)
    print("RESULT " + json.dumps([rcs, reported, digest.hexdigest()[:16]]), flush=True)


def observe(case):
    """[[return codes, reported level-1 kernel, digest], forward launches as 'kernel XxYxZ block']"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["HIPEMU_TRACE"] = "1"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "child", case], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    result = json.loads(next(line for line in run.stdout.splitlines() if line.startswith("RESULT "))[7:])
    launched = []
    for line in run.stderr.splitlines():
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)  block (\d+) ", line)
        if not m: continue
        kernel = m.group(1).rsplit("::", 1)[-1]
        if FORWARD.match(kernel): launched.append("%s%s %sx%sx%s %s" % (kernel, m.group(2) or "", m.group(3), m.group(4), m.group(5), m.group(6)))
    return [result, launched]


@pytest.mark.parametrize("case", sorted(CASES))
def test_input_route_launches_what_was_recorded(case):
    with open(GOLDEN) as fh: expected = json.load(fh)
    assert sorted(expected) == sorted(CASES), "CASES and the recorded table name different cases"
    seen = observe(case)
    print("expected", expected[case], "\nobserved", seen)
    assert seen == expected[case]
    want = "k_fwd_gop_packed16" if CASES[case][1] & GOP else "k_fwd_packed16"
    assert seen[0][1] == want and seen[1][0].startswith(want + " "), "the reported level-1 kernel is the first one launched"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "child": _child(sys.argv[2])
    else:
        with open(GOLDEN, "w") as fh: fh.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(c), json.dumps(observe(c))) for c in sorted(CASES)) + "\n}\n")
