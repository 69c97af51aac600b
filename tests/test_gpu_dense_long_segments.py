"""Long segments for the densely counted bands on the real kernels (run with `pytest -m gpu` on an MI355X): batches of 8 frames -- the smallest count that takes the
many-frame launch path of GpuEntropyEncoder::launch (act >= 8) -- through cfhd_amd_batch_create_ex, at the shapes of tests/test_entropy_dense_long_segments.py:

  512 x 272 YUY2: level 2 of 8704 / 4352 coefficients, level 3 of 2176 / 1088; level 1 from block lists.  Round trip: every decoded picture inside the oracle's dither interval.
  256 x 136 RG48 (RGB 4:4:4): level-1 bands of 8704 coefficients counted densely.  Encode only.

Every sample against the reference encoder's sample of its frame, counters and clock metadata masked, for the default lengths and for every value {1024, 2048, 4096, 8192}
of each switch that reaches the shape (CFHD_AMD_SEG_L2, CFHD_AMD_SEG_L3, and CFHD_AMD_SEG_L1_DENSE for RG48; read at every prepare: one process holds them all).

A pass of 8 such frames does not fill the chip, so its default is 1024 everywhere (GpuEntropyEncoder::prepare_units); the switches hold at any size.  The default lengths of a
pass that does fill it are taken by one more batch per shape, of as many frames as that needs (8192 segments of 1024 coefficients), held to the same reference samples.

Each shape runs in a fresh child process under a time limit of its own; once one has failed, the other does not touch the GPU."""
import ctypes, os, subprocess, sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1024, 2048, 4096, 8192)
SWITCHES = {"yuy2": ("CFHD_AMD_SEG_L2", "CFHD_AMD_SEG_L3"), "rg48": ("CFHD_AMD_SEG_L1_DENSE", "CFHD_AMD_SEG_L2", "CFHD_AMD_SEG_L3")}
NFRAMES = 8
_failed = []

pytestmark = pytest.mark.gpu


def worker(shape):
    sys.path.insert(0, HERE)
    import cfhd_testlib as T
    from test_gpu_parity import _batch_api
    assert T.have_ref(), "oracle/_ref/libcfhd_ref.so is needed: the samples are compared with the reference encoder's"
    L = _batch_api()
    if shape == "yuy2":
        w, h, fmt, enc, mode, bpp = 512, 272, T.PIX_YUY2, T.ENCODED_YUV422, 0, 2
        q, pitch = T.qbist_frames(10, 2, w, h)
        uniq = [q[0], q[1], T.synth_yuy2(w, h, 3)[0]]
    else:
        w, h, fmt, enc, mode, bpp = 256, 136, T.PIX_RG48, T.ENCODED_RGB444, 1, 6
        uniq, pitch = T.qbist_frames(10, 3, w, h, T.PIX_RG48)
    assert pitch == w * bpp
    plan0 = T.Plan(w, h) if shape == "yuy2" else T.Plan(w, h, pixkind=T.PIXKIND["RG48"], enc=T.ENC["444"])
    nbig = 8192 * 1024 // plan0.coeff_elems + 2              # frames of a pass that fills the chip: the default lengths apply
    frames = [uniq[i % len(uniq)] for i in range(nbig)]
    refs = [T.mask_volatile_metadata(r) for r in T.ref_encode_frames(frames, pitch, w, h, fmt, encoded=enc)]      # once: one reference encoder, consecutive calls
    interval = {}
    settings = [(NFRAMES, {})] + [(NFRAMES, {name: str(v)}) for name in SWITCHES[shape] for v in LENGTHS] + [(nbig, {})]
    for n, env in settings:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            b = L.cfhd_amd_batch_create_ex(w, h, fmt, enc, 0, T.QUALITY_FILMSCAN1, n, 4, mode)
            assert b, T.amd_last_error()
            for i, f in enumerate(frames[:n]):
                assert L.cfhd_amd_batch_upload(b, i, f.ctypes.data_as(ctypes.c_void_p), pitch) == 0
            assert L.cfhd_amd_batch_roundtrip(b) > 0, T.amd_last_error()
            for i in range(n):
                p = ctypes.c_void_p(); sz = ctypes.c_size_t()
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                sample = ctypes.string_at(p, sz.value)
                assert len(sample) == len(refs[i]), "%s frame %d: %d bytes vs reference %d" % (env, i, len(sample), len(refs[i]))
                assert T.mask_volatile_metadata(sample) == refs[i], "%s frame %d differs from the reference" % (env, i)
                if mode: continue
                out = np.zeros(h * w * 2, np.uint8)
                assert L.cfhd_amd_batch_download_output(b, i, out.ctypes.data_as(ctypes.c_void_p), 2 * w) == 0
                k = i % len(uniq)
                if k not in interval:
                    plan = T.Plan(w, h)
                    deq = T.oracle_decode_pyramid(sample, plan)
                    interval[k] = (T.oracle_inverse_yuv422(plan, deq, 0)[:h], T.oracle_inverse_yuv422(plan, deq, 1)[:h])
                lo, hi = interval[k]
                img = out.reshape(h, 2 * w)
                ok = (img == lo) | (img == hi)
                assert ok.all(), "%s frame %d: %d bytes outside the dither interval" % (env, i, (~ok).sum())
            L.cfhd_amd_batch_destroy(b)
        finally:
            for k, v in old.items():
                if v is None: os.environ.pop(k, None)
                else: os.environ[k] = v
        print("ok", shape, n, "frames", env or "defaults", flush=True)
    print("done", shape, len(settings), "settings", flush=True)


@pytest.mark.parametrize("shape", ["yuy2", "rg48"])
def test_batched_samples_equal_reference_at_every_segment_length(shape):
    if _failed: pytest.fail("not run: the child process of %s failed before" % _failed[0])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--worker", shape]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    except subprocess.TimeoutExpired as e:
        _failed.append(shape)
        pytest.fail("time limit: %s" % (e.stdout or b"").decode(errors="replace")[-2000:])
    text = r.stdout.decode(errors="replace")
    print(text)
    if r.returncode != 0 or ("done " + shape) not in text:
        _failed.append(shape)
        pytest.fail("child process ended with %d:\n%s" % (r.returncode, text[-3000:]))


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--worker"
    worker(sys.argv[2])
