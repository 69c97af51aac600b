"""Every launch of the GPU entropy stage -- coder and decoder, each job source, back-end and count arrangement -- against what it launched before, on the emulated
product library.

Each case runs in a fresh child interpreter with HIPEMU_TRACE=1 (the emulator reads it, and the entropy stage reads several of its switches, once per process) and
does one cfhd_amd_batch_roundtrip of YUY2 frames.  The emulator's launch trace (tests/hipemu/hip/hip_runtime.h launch_sync) is the witness: per case the test
asserts the return code, the exact sequence of the k_ent_* / k_dec_* launches (kernel, grid, block) and, of a pass that succeeded, one digest over the samples
(volatile metadata masked) and one over the decoded pictures.  A pass the library refuses is pinned as its return code.

tests/golden/entropy_launches.json was recorded (`python tests/test_entropy_launches_emulated.py record`) on the commit before the entropy stage's host side got one
launch path (cfhd_entropy_gpu.hip: DecBackend, GpuEntropyDecoder::launch, the count stage of GpuEntropyEncoder::launch), not from the code it now checks: which
kernels a pass launches, in which order and over which grids, must not move when the code that decides it does.  192x96 is test_output_routes_emulated.py's size;
33 frames cross the decoder's kLowLatencyFrames (k_dec_bands_par instead of k_dec_bands_par_ll), 8 frames reach the coder's split count stage and the decoder's
split tile pass.  The emulated batch gives the coder's two streams as one (cfhd_batch.cpp StreamScope) unless CFHD_AMD_STREAMS=3.

Test infrastructure only: nothing here is a product path."""
import ctypes, hashlib, json, os, re, subprocess, sys
import numpy as np
import pytest

W, H = 192, 96
INTERLACED = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entropy_launches.json")
DEVICE, HOST = {"CFHD_AMD_HANDOFF": "device"}, {"CFHD_AMD_HANDOFF": "host"}
PAR, LANE = {"CFHD_AMD_DEC": "par"}, {"CFHD_AMD_DEC": "lane"}
FWD_STRIP, INV_STRIP = {"CFHD_AMD_FORWARD": "strip"}, {"CFHD_AMD_INVERSE": "strip"}      # (the block lists of either side belong to the strip kernels: by size only from 32 frames of 1080p on)
# name: (frames, encoding flags, environment)
CASES = {
    "device-dx": (2, 0, DEVICE), "device-par": (2, 0, dict(DEVICE, **PAR)), "device-lane": (2, 0, dict(DEVICE, **LANE)),
    "host-dx": (2, 0, HOST), "host-par": (2, 0, dict(HOST, **PAR)), "host-lane": (2, 0, dict(HOST, **LANE)),
    "device-dx-repair": (2, 0, dict(DEVICE, CFHD_AMD_DX_SPECULATE="0")),
    "device-par-33": (33, 0, dict(DEVICE, **PAR)), "host-par-33": (33, 0, dict(HOST, **PAR)),
    "interlaced-device-dx": (2, INTERLACED, DEVICE), "interlaced-host-dx": (2, INTERLACED, HOST),
    "interlaced-device-par": (2, INTERLACED, dict(DEVICE, **PAR)), "interlaced-host-par": (2, INTERLACED, dict(HOST, **PAR)),
    "count-8": (8, 0, DEVICE), "count-8-unsplit": (8, 0, dict(DEVICE, CFHD_AMD_COUNT_SPLIT="0")), "count-8-dense": (8, 0, dict(DEVICE, CFHD_AMD_BLOCKS="0")),
    "count-8-lists": (8, 0, dict(DEVICE, **FWD_STRIP)), "count-8-lists-unsplit": (8, 0, dict(DEVICE, CFHD_AMD_COUNT_SPLIT="0", **FWD_STRIP)),
    "count-8-lists-off": (8, 0, dict(DEVICE, CFHD_AMD_BLOCKS="0", **FWD_STRIP)), "count-8-lists-off-unsplit": (8, 0, dict(DEVICE, CFHD_AMD_BLOCKS="0", CFHD_AMD_COUNT_SPLIT="0", **FWD_STRIP)),
    "count-8-lists-three-streams": (8, 0, dict(DEVICE, CFHD_AMD_STREAMS="3", **FWD_STRIP)),
    "dec-blocks-off": (2, 0, dict(DEVICE, CFHD_AMD_DEC_BLOCKS="0")), "dec-lists": (2, 0, dict(DEVICE, **INV_STRIP)),
    "dec-lists-off": (2, 0, dict(DEVICE, CFHD_AMD_DEC_BLOCKS="0", **INV_STRIP)), "dec-lists-host": (2, 0, dict(HOST, **INV_STRIP)),
    "tiles-split-device": (8, 0, dict(DEVICE, CFHD_AMD_TILES_SPLIT="1")), "tiles-split-host": (8, 0, dict(HOST, CFHD_AMD_TILES_SPLIT="1")),
}
ENTROPY = re.compile(r"k_(ent|dec)_")


def _child(case):
    """One batch and one pass; 'RESULT <json>' ([return code, digest of the samples, digest of the pictures]) on stdout, the trace on stderr."""
    import cfhd_testlib as T
    frames, flags, _ = CASES[case]
    with T.emulated_product() as L:
        L.cfhd_amd_batch_create_ex.restype = ctypes.c_void_p
        L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.cfhd_amd_batch_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.cfhd_amd_batch_roundtrip.restype = ctypes.c_longlong
        L.cfhd_amd_batch_roundtrip.argtypes = [ctypes.c_void_p]
        L.cfhd_amd_batch_get_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.cfhd_amd_batch_download_output.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.cfhd_amd_batch_destroy.argtypes = [ctypes.c_void_p]
        b = L.cfhd_amd_batch_create_ex(W, H, T.PIX_YUY2, T.ENCODED_YUV422, flags, T.QUALITY_FILMSCAN1, frames, 1, 0)
        assert b, T.amd_last_error()
        for i in range(frames):
            frame, pitch = T.synth_yuy2(W, H, 7 + i)
            assert L.cfhd_amd_batch_upload(b, i, frame.ctypes.data_as(ctypes.c_void_p), pitch) == 0
        rc = L.cfhd_amd_batch_roundtrip(b)
        samples, pictures = hashlib.sha256(), hashlib.sha256()
        for i in range(frames if rc > 0 else 0):
            p = ctypes.c_void_p(); sz = ctypes.c_size_t()
            assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
            samples.update(T.mask_volatile_metadata(ctypes.string_at(p, sz.value)))
            out = np.zeros(H * W * 2, dtype=np.uint8)
            assert L.cfhd_amd_batch_download_output(b, i, out.ctypes.data_as(ctypes.c_void_p), W * 2) == 0
            pictures.update(out.tobytes())
        L.cfhd_amd_batch_destroy(b)
    print("RESULT " + json.dumps([rc if rc < 0 else 0] + ([samples.hexdigest()[:16], pictures.hexdigest()[:16]] if rc > 0 else [])), flush=True)


def observe(case):
    """[[return code (0: a pass that succeeded), digests], entropy launches as 'kernel XxYxZ block']"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env.update(CASES[case][2], HIPEMU_TRACE="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "child", case], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    result = json.loads(next(line for line in run.stdout.splitlines() if line.startswith("RESULT "))[7:])
    launched = []
    for line in run.stderr.splitlines():
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+)  block (\d+) ", line)
        if not m: continue
        kernel = m.group(1).rsplit("::", 1)[-1]
        if ENTROPY.match(kernel): launched.append("%s %sx%sx%s %s" % (kernel, m.group(3), m.group(4), m.group(5), m.group(6)))
    return [result, launched]


@pytest.mark.parametrize("case", sorted(CASES))
def test_entropy_stage_launches_what_it_launched_before(case):
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
