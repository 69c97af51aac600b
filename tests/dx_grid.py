"""The grids of the chunk-indexed decoder's persistent kernels (k_dec_index, k_dec_reindex, k_dec_tiles) must never change a result: shared by
tests/test_dx_grid_emulated.py (CPU, the emulated product and the emulated kernels) and tests/test_gpu_dx_grid.py (the hardware).

The batch: four synthetic 4:2:2 frames at 320 x 192 -- the width a multiple of 32, so the level-1 bands leave k_dec_tiles as block lists; a few dozen 2016-byte chunks
and a handful of tiles per frame -- through one frame-queue batch, encode and decode.  The hand-made samples (tests/hand_made_samples.py) go through a fresh decoder
handle each.  The grids are forced by CFHD_AMD_DX_GRID_INDEX / CFHD_AMD_DX_GRID_TILES, which a decoder reads when it is prepared."""
import ctypes, functools, os
import numpy as np
from cfhd_testlib import *
import hand_made_samples as S

W, H, N = 320, 192, 4
V = ctypes.c_void_p


class forced_grids:
    """CFHD_AMD_DX_GRID_INDEX = CFHD_AMD_DX_GRID_TILES = grid for decoders prepared inside (None: the library's own shapes); speculate=False: CFHD_AMD_DX_SPECULATE=0,
    every chunk but a band's first through k_dec_chain / k_dec_repair / k_dec_reindex.  Always CFHD_AMD_INVERSE=strip: small launches too leave the level-1 bands as
    block lists with occupancy masks for k_inv_yuv422_strip_blocks, as the large ones do by themselves."""
    NAMES = ("CFHD_AMD_DX_GRID_INDEX", "CFHD_AMD_DX_GRID_TILES", "CFHD_AMD_DX_SPECULATE", "CFHD_AMD_INVERSE")

    def __init__(self, grid, speculate=True):
        self.values = {"CFHD_AMD_DX_GRID_INDEX": grid, "CFHD_AMD_DX_GRID_TILES": grid, "CFHD_AMD_DX_SPECULATE": None if speculate else "0",
                       "CFHD_AMD_INVERSE": "strip"}

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.NAMES}
        for k, v in self.values.items():
            os.environ.pop(k, None)
            if v is not None: os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.before.items():
            os.environ.pop(k, None)
            if v is not None: os.environ[k] = v


@functools.lru_cache(maxsize=None)
def frames():
    """The four frames (computed once, shared, read-only)."""
    out = [synth_yuy2(W, H, 50 + i)[0] for i in range(N)]
    for f in out: f.setflags(write=False)
    return tuple(out)


def batch_api():
    L = product()
    L.cfhd_amd_batch_create.restype = V
    L.cfhd_amd_batch_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.cfhd_amd_batch_upload.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
    for f in (L.cfhd_amd_batch_roundtrip, L.cfhd_amd_batch_wait): f.restype = ctypes.c_longlong; f.argtypes = [V]
    L.cfhd_amd_batch_submit.argtypes = [V]
    L.cfhd_amd_batch_get_sample.argtypes = [V, ctypes.c_int, ctypes.POINTER(V), ctypes.POINTER(ctypes.c_size_t)]
    L.cfhd_amd_batch_download_output.argtypes = [V, ctypes.c_int, V, ctypes.c_int]
    L.cfhd_amd_batch_destroy.argtypes = [V]; L.cfhd_amd_batch_destroy.restype = None
    return L


def upload(L, b, i, frame, pitch):
    assert L.cfhd_amd_batch_upload(b, i, np.ascontiguousarray(frame).ctypes.data_as(V), pitch) == 0, amd_last_error()


def batch_round_trip(grid, speculate=True):
    """One pass of the batch under the forced grids: ([sample bytes], [YUY2 picture as (H, 2 W) bytes])."""
    L = batch_api()
    with forced_grids(grid, speculate):
        b = L.cfhd_amd_batch_create(W, H, PIX_YUY2, QUALITY_FILMSCAN1, N, 1)
        assert b, amd_last_error()
        try:
            for i, f in enumerate(frames()): upload(L, b, i, f, W * 2)
            total = L.cfhd_amd_batch_roundtrip(b)
            assert total > 0, "pass -> %d (%s)" % (total, amd_last_error())      # (< 0: among others the decoder's error word, -7)
            samples, pictures = [], []
            for i in range(N):
                p = V(); n = ctypes.c_size_t()
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(n)) == 0
                samples.append(ctypes.string_at(p, n.value))
                o = np.full(H * W * 2, 7, np.uint8)
                assert L.cfhd_amd_batch_download_output(b, i, o.ctypes.data_as(V), W * 2) == 0, amd_last_error()
                pictures.append(o.reshape(H, W * 2))
        finally:
            L.cfhd_amd_batch_destroy(b)
    return samples, pictures


@functools.lru_cache(maxsize=None)
def want_samples():
    """The batch's samples by the oracle's transform and the host writer (frame numbers 1 .. N), without their metadata: the sample's own is spliced in by the caller."""
    plan = Plan(W, H)
    return plan, tuple(oracle_forward_yuv422(plan, f, W * 2) for f in frames())


def check_batch(samples, pictures, what):
    """Samples byte for byte the oracle + host writer; every picture inside the oracle's dither interval of its sample's pyramid."""
    plan, coeffs = want_samples()
    for i in range(N):
        off, m = first_metadata_chunk(samples[i])
        assert samples[i] == product_write_sample_host(plan, coeffs[i], i + 1, meta_global=samples[i][off:off + m]), "%s: sample %d differs from the oracle + host writer" % (what, i)
        lo, hi = batch_interval(i, samples[i])
        ok = (pictures[i] == lo) | (pictures[i] == hi)
        assert ok.all(), "%s: picture %d leaves the oracle's dither interval in %d bytes, first at %s" % (what, i, (~ok).sum(), tuple(np.argwhere(~ok)[0]))


@functools.lru_cache(maxsize=None)
def batch_interval(i, sample):
    plan = Plan(W, H)
    deq = oracle_decode_pyramid(sample, plan)
    return oracle_inverse_yuv422(plan, deq, 0)[:H], oracle_inverse_yuv422(plan, deq, 1)[:H]


def _without_metadata(sample):
    """(the global block carries the encoder's clock and a GUID per process: every pass writes its own)"""
    off, m = first_metadata_chunk(sample)
    return sample[:off] + sample[off + m:]


def same_batches(a, b, what):
    for i in range(N):
        assert _without_metadata(a[0][i]) == _without_metadata(b[0][i]), "%s: sample %d differs" % (what, i)
        bad = a[1][i] != b[1][i]
        assert not bad.any(), "%s: picture %d differs in %d bytes, first at %s" % (what, i, bad.sum(), tuple(np.argwhere(bad)[0]))


def hand_made_yuy2(name, grid, speculate=True):
    """The YUY2 picture of a hand-made sample through a fresh decoder handle prepared under the forced grids."""
    c = S.case(name)
    with forced_grids(grid, speculate):
        got, pitch, aw, ah = amd_decode_sample(c.sample, PIX_YUY2)
    assert (aw, ah) == (c.w, c.h)
    return got.reshape(c.h, pitch)[:, : c.w * 2].copy()


def check_hand_made(name, grids, speculate=True):
    """Inside the oracle's interval under the first grid, byte-identical under the others: the dither is the library's hash of the position, so a coefficient or a block
    that moved shows even inside the interval."""
    first = hand_made_yuy2(name, grids[0], speculate)
    lo, hi = S.want_yuy2_interval(name)
    ok = (first == lo) | (first == hi)
    assert ok.all(), "%s, grid %s: %d bytes outside the oracle's dither interval" % (name, grids[0], (~ok).sum())
    for g in grids[1:]:
        bad = hand_made_yuy2(name, g, speculate) != first
        assert not bad.any(), "%s: grid %s and grid %s give different pictures in %d bytes, first at %s" % (name, g, grids[0], bad.sum(), tuple(np.argwhere(bad)[0]))
