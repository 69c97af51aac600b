"""The kernel names a batch reports (cfhd_amd_batch_kernel_name) against the kernels it launches, on the emulated product library.

The GPU tests and bench.py take the reported name as their proof of which transform kernel ran.  Here the emulator's launch trace (HIPEMU_TRACE: one line per
launch on stderr, tests/hipemu/hip/hip_runtime.h launch_sync) is the witness: for every case the sequence of transform launches of one pass must equal the
reported names in launch order.  The emulator reads HIPEMU_TRACE once per process and the forward side reads CFHD_AMD_BLOCKS once per process, so every case
runs in a fresh child interpreter with its switches set from the start.  The library is compared with itself: no reference library is needed.

Test infrastructure only: nothing here is a product path."""
import ctypes, json, os, re, subprocess, sys
import numpy as np
import pytest

SHAPES = ("CFHD_AMD_FORWARD", "CFHD_AMD_INVERSE", "CFHD_AMD_PLANES")
TILE, STRIP = {k: "tile" for k in SHAPES}, {k: "strip" for k in SHAPES}
# name: (width, height, pixel format, encoded format, encoding flags, batch mode (1: encode only), environment) -- the sizes tests/test_product_emulated.py emulates (ALWAYS there)
CASES = {
    "yuy2-by-size": (1952, 250, "YUY2", "422", 0, 0, {}),
    "yuy2-tile": (1952, 250, "YUY2", "422", 0, 0, TILE),
    "yuy2-strip": (1952, 250, "YUY2", "422", 0, 0, STRIP),
    "yuy2-strip-two-segments": (2304, 72, "YUY2", "422", 0, 0, STRIP),
    "yuy2-strip-dense-encode": (1952, 250, "YUY2", "422", 0, 0, dict(STRIP, CFHD_AMD_BLOCKS="0")),
    "yuy2-strip-dense-decode": (1952, 250, "YUY2", "422", 0, 0, dict(STRIP, CFHD_AMD_DEC_BLOCKS="0")),
    "interlaced-tile": (2048, 120, "YUY2", "422", 1, 0, TILE),
    "interlaced-strip": (2048, 120, "YUY2", "422", 1, 0, STRIP),
    "rg48-tile": (504, 242, "RG48", "444", 0, 0, TILE),
    "rg48-strip": (504, 242, "RG48", "444", 0, 0, STRIP),
    "b64a-tile": (136, 120, "b64a", "4444", 0, 0, TILE),
    "b64a-strip": (136, 120, "b64a", "4444", 0, 0, STRIP),
    "byr4-encode-tile": (1008, 244, "BYR4", "bayer", 0, 1, TILE),
    "byr4-encode-strip": (1008, 244, "BYR4", "bayer", 0, 1, STRIP),
}
FRAMES = 2
TRANSFORM = re.compile(r"k_(fwd|unpack|inv|half)_")


def _child(case):
    """One batch, its six kernel names (asked before the first launch, as the GPU tests ask) and one pass; the names go to stdout as JSON, the trace to stderr."""
    import cfhd_testlib as T
    w, h, fmt, enc, flags, mode, _ = CASES[case]
    fourcc = {"YUY2": T.PIX_YUY2, "RG48": T.PIX_RG48, "b64a": T.PIX_B64A, "BYR4": T.PIX_BYR4}[fmt]
    encoded = {"422": T.ENCODED_YUV422, "444": T.ENCODED_RGB444, "4444": T.ENCODED_RGBA4444, "bayer": T.ENCODED_BAYER}[enc]
    with T.emulated_product() as L:
        L.cfhd_amd_batch_create_ex.restype = ctypes.c_void_p
        L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.cfhd_amd_batch_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.cfhd_amd_batch_roundtrip.restype = ctypes.c_longlong
        L.cfhd_amd_batch_roundtrip.argtypes = [ctypes.c_void_p]
        L.cfhd_amd_batch_kernel_name.restype = ctypes.c_char_p
        L.cfhd_amd_batch_kernel_name.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.cfhd_amd_batch_destroy.argtypes = [ctypes.c_void_p]
        b = L.cfhd_amd_batch_create_ex(w, h, fourcc, encoded, flags, T.QUALITY_FILMSCAN1, FRAMES, 1, mode)
        assert b, T.amd_last_error()
        for i in range(FRAMES):
            if fmt == "YUY2": frame, pitch = T.synth_yuy2(w, h, 7 + i)
            elif fmt == "BYR4": frame, pitch = T.synth_bayer(w, h, 7 + i).reshape(-1).view(np.uint8).copy(), w * 2
            else:
                words = {"RG48": 3, "b64a": 4}[fmt]
                y, x = np.mgrid[0:h, 0:w * words]
                frame = ((np.sin(x / 29.0 + i) * np.cos(y / 17.0) * 0.4 + 0.5) * 60000 + (x * y % 977)).astype(np.uint16).reshape(-1).view(np.uint8).copy()
                pitch = w * words * 2
            assert L.cfhd_amd_batch_upload(b, i, frame.ctypes.data_as(ctypes.c_void_p), pitch) == 0
        names = [L.cfhd_amd_batch_kernel_name(b, slot).decode() for slot in range(6)]
        assert L.cfhd_amd_batch_roundtrip(b) > 0, T.amd_last_error()
        L.cfhd_amd_batch_destroy(b)
    print("NAMES " + json.dumps(names))


def _collapsed(seq):
    return [k for i, k in enumerate(seq) if i == 0 or k != seq[i - 1]]


@pytest.mark.parametrize("case", sorted(CASES))
def test_reported_kernel_names_are_the_launched_kernels(case):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env.update(CASES[case][6], HIPEMU_TRACE="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    names = json.loads(next(line for line in run.stdout.splitlines() if line.startswith("NAMES "))[6:])
    # the launch order of a pass: forward levels 1, 2, 3 (slots 0, 1, 2), inverse levels 3, 2 and the last one (slots 5, 4, 3); "a+b" is two launches
    reported = _collapsed([k for slot in (0, 1, 2, 5, 4, 3) for k in names[slot].split("+") if k])
    launched = []
    for line in run.stderr.splitlines():
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid ", line)
        if not m: continue
        kernel = m.group(1).rsplit("::", 1)[-1]
        if TRANSFORM.match(kernel): launched.append(kernel)
    launched = _collapsed(launched)
    print("reported", reported, "\nlaunched", launched)
    assert launched, "no transform launch in the trace"
    assert CASES[case][5] == 1 or any(k.startswith(("k_inv_", "k_half_")) for k in launched), "a round trip without an inverse launch"
    assert launched == reported


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[1])
