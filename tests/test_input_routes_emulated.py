"""Every encoder input route -- pixel format x encoded format x scan x shape switch, intra batches and two-frame groups -- against what it launched before, on the
emulated product library.

Each case runs in a fresh child interpreter with HIPEMU_TRACE=1 (the emulator reads it, and the forward side reads CFHD_AMD_BLOCKS, once per process).  An intra case
is one encode-only cfhd_amd_batch_roundtrip of two frames, a group case two CFHD_EncodeSample calls of a two-frame group encoder.  The emulator's launch trace
(tests/hipemu/hip/hip_runtime.h launch_sync) is the witness: per case the test asserts the return codes, the exact sequence of the k_fwd_* / k_unpack_byr4 / k_gop_*
launches (kernel, grid, block), the level-1 kernel the batch or the encoder reports (cfhd_amd_batch_kernel_name / cfhd_amd_encoder_kernel_name, asked before the first
launch) and one digest over the samples, volatile metadata masked.

tests/golden/input_routes.json was recorded (`python tests/test_input_routes_emulated.py record`) on the commit before the encoder's first level got one launcher and
one filler per job family (cfhd_device.hip launch_first_level, fill_fwd_yuv_job, fill_fwd_plane_job; cfhd_kernels.h FwdLayout), not from the code it now checks: which
kernels an input launches, over which grids, and the bytes they leave must not move when the code that fills the job tables and launches them does.  The sizes are
those the CPU suite emulates already: 192x96 (test_output_routes_emulated.py), the strip rows of test_launch_routes_emulated.py, and 320x240 for a group whose tile
rows hold three luma and two chroma tiles in k_fwd_gop_packed16.

Test infrastructure only: nothing here is a product path."""
import ctypes, hashlib, json, os, re, subprocess, sys
import numpy as np
import pytest

W, H = 192, 96
GOP, INTERLACED = 2, 1      # encoding flags
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "input_routes.json")
STRIP = {"CFHD_AMD_FORWARD": "strip", "CFHD_AMD_PLANES": "strip"}
GOP_INPUTS = ("YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a", "RG64", "YUY2")      # (the formats of tests/gop_input_frames.py)
# name: (width, height, pixel format, encoded format, encoding flags, environment); the GOP flag: a group encoder of the C ABI instead of a batch
CASES = {}
for f in ("YUY2", "2vuy", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a"): CASES["422 " + f] = (W, H, f, "422", 0, {})
for f in ("RG24", "BGRA", "r210", "DPX0", "AB10", "RG48", "b64a", "RG64"): CASES["444 " + f] = (W, H, f, "444", 0, {})
for f in ("BGRA", "b64a", "RG64"): CASES["4444 " + f] = (W, H, f, "4444", 0, {})
for f in ("BYR4", "BYR5"): CASES["bayer " + f] = (W, H, f, "bayer", 0, {})
CASES["422i YUY2"] = (W, H, "YUY2", "422", INTERLACED, {})
CASES.update({
    "strip 422 YUY2": (1952, 250, "YUY2", "422", 0, STRIP), "strip 422 YUY2 two segments": (2304, 72, "YUY2", "422", 0, STRIP),
    "strip 422i YUY2": (2048, 120, "YUY2", "422", INTERLACED, STRIP), "strip 444 RG48": (504, 242, "RG48", "444", 0, STRIP),
    "strip 4444 b64a": (136, 120, "b64a", "4444", 0, STRIP), "strip bayer BYR4": (1008, 244, "BYR4", "bayer", 0, STRIP),
    "strip 422 YUY2 blocks=0": (1952, 250, "YUY2", "422", 0, dict(STRIP, CFHD_AMD_BLOCKS="0")),
})
for f in GOP_INPUTS: CASES["gop " + f] = (W, H, f, "422", GOP, {})
CASES["gopi YUY2"] = (W, H, "YUY2", "422", GOP | INTERLACED, {})
CASES["gop v210 320x240"] = (320, 240, "v210", "422", GOP, {})
FRAMES = 2
FORWARD = re.compile(r"k_fwd_|k_unpack_byr4$|k_gop_")


def _frame(fmt, w, h, seed):
    """(bytes of one frame as a uint8 array, pitch in bytes)"""
    import cfhd_testlib as T
    import gop_input_frames as G
    if fmt == "2vuy": return T.synth_yuy2(w, h, seed)      # (the same bytes read as U Y V Y)
    if fmt == "BYR4": return T.synth_bayer(w, h, seed).reshape(-1).view(np.uint8).copy(), w * 2
    if fmt == "BYR5": return T.pack_byr5(T.synth_bayer(w, h, seed)), w * 3
    if fmt in T.RGB10_FORMATS:
        order, shifts, _ = T.RGB10_FORMATS[fmt]
        rng = np.random.default_rng(seed)
        words = sum((G._component(rng, w, h, seed, k) * 1023).astype(np.uint32) << s for k, s in enumerate(shifts))
        return words.astype(order + "u4").view(np.uint8).reshape(-1).copy(), w * 4
    return G.frame(fmt, w, h, seed)


def _child(case):
    """'RESULT <json>' ([return codes, reported level-1 kernel, digest of the samples]) on stdout, the trace on stderr."""
    import cfhd_testlib as T
    w, h, fmt, enc, flags, _ = CASES[case]
    encoded = {"422": T.ENCODED_YUV422, "444": T.ENCODED_RGB444, "4444": T.ENCODED_RGBA4444, "bayer": T.ENCODED_BAYER}[enc]
    frames = [_frame(fmt, w, h, 7 + i) for i in range(FRAMES)]
    pitch = frames[0][1]
    digest, rcs = hashlib.sha256(), []
    with T.emulated_product() as L:
        if flags & GOP:
            L.cfhd_amd_encoder_kernel_name.restype = ctypes.c_char_p
            L.cfhd_amd_encoder_kernel_name.argtypes = [ctypes.c_void_p]
            enc_h = ctypes.c_void_p(); assert L.CFHD_OpenEncoder(ctypes.byref(enc_h), None) == 0
            rcs.append(L.CFHD_PrepareToEncode(enc_h, w, h, T.fourcc(fmt), encoded, flags, T.QUALITY_FILMSCAN1))
            name = L.cfhd_amd_encoder_kernel_name(enc_h).decode()
            for f, _ in frames if rcs[0] == 0 else []:
                rcs.append(L.CFHD_EncodeSample(enc_h, f.ctypes.data_as(ctypes.c_void_p), pitch))
                if rcs[-1]: break
                p = ctypes.c_void_p(); n = ctypes.c_size_t()
                assert L.CFHD_GetSampleData(enc_h, ctypes.byref(p), ctypes.byref(n)) == 0
                digest.update(T.mask_volatile_metadata(ctypes.string_at(p, n.value)))
            L.CFHD_CloseEncoder(enc_h)
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
            b = L.cfhd_amd_batch_create_ex(w, h, T.fourcc(fmt), encoded, flags, T.QUALITY_FILMSCAN1, FRAMES, 1, 1)      # (mode 1: encode only)
            assert b, T.amd_last_error()
            for i, (f, _) in enumerate(frames): assert L.cfhd_amd_batch_upload(b, i, f.ctypes.data_as(ctypes.c_void_p), pitch) == 0
            name = L.cfhd_amd_batch_kernel_name(b, 0).decode()
            rc = L.cfhd_amd_batch_roundtrip(b)
            rcs.append(rc if rc < 0 else 0)
            for i in range(FRAMES if rc > 0 else 0):
                p = ctypes.c_void_p(); sz = ctypes.c_size_t()
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                digest.update(T.mask_volatile_metadata(ctypes.string_at(p, sz.value)))
            L.cfhd_amd_batch_destroy(b)
    print("RESULT " + json.dumps([rcs, name, digest.hexdigest()[:16]]), flush=True)


def observe(case):
    """[[return codes, reported level-1 kernel, digest], forward launches as 'kernel XxYxZ block']"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env.update(CASES[case][5], HIPEMU_TRACE="1")
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
def test_input_route_launches_what_it_launched_before(case):
    with open(GOLDEN) as fh: expected = json.load(fh)
    assert sorted(expected) == sorted(CASES), "CASES and the recorded table name different cases"
    seen = observe(case)
    print("expected", expected[case], "\nobserved", seen)
    assert seen == expected[case]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "child": _child(sys.argv[2])
    else:
        with open(GOLDEN, "w") as fh: fh.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(c), json.dumps(observe(c))) for c in sorted(CASES)) + "\n}\n")
