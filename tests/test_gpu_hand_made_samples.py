"""Hand-made code streams through the chunk-indexed decoder on the real kernels (run with `pytest -m gpu` on an MI355X; tests/test_hand_made_samples.py pins the cases
on the CPU and runs every body below on the emulated product).

The rest of the GPU suite feeds k_dec_plan / k_dec_index / k_dec_chain / k_dec_repair / k_dec_reindex / k_dec_tile_index / k_dec_tiles what an encoder made from a
picture.  Here the host writer makes the samples from hand-made pyramids (tests/hand_made_samples.py): bands without a unique alignment, zero runs of 3072 and more
across chunk and tile boundaries, values on the last coefficient of tile 0 and the first of tile 1, payloads that end at a multiple of 2016 bytes, a tile that fills the LDS image, frames whose bands
hold from one chunk to many gathered into one launch.  What the emulation cannot see -- a missing barrier, a race on the shared tile image, an ordering assumption of
the persistent index loop, a wrong wait count -- shows here or nowhere.

Witness: a 4:2:2 sample decoded to YU64 is a word-exact, dither-free image of the decoded pyramid (oracle_inverse_yu64 of oracle_decode_pyramid, pinned on the
reference by test_oracle_vs_ref); test_hand_made_samples.py asserts that at least 95 % of single-coefficient errors change that image.  Every sample is well-formed and
goes through the C ABI on a fresh decoder handle; no reference call."""
import ctypes, os, threading
import numpy as np
import pytest
from cfhd_testlib import *
import hand_made_samples as S

pytestmark = pytest.mark.gpu
REPAIR_CASES = ("dense_small", "constant", "long_runs", "chunk_edges")


def _yu64(name, decoder=None):
    c = S.case(name)
    got, pitch, aw, ah = amd_decode_sample(c.sample, fourcc("YU64"), decoder=decoder)
    assert (aw, ah) == (c.w, c.h)
    return np.frombuffer(got.tobytes(), np.uint16).reshape(c.h, pitch // 2)[:, : c.w * 2]


def _yuy2(name, decoder=None):
    c = S.case(name)
    got, pitch, aw, ah = amd_decode_sample(c.sample, PIX_YUY2, decoder=decoder)
    assert (aw, ah) == (c.w, c.h)
    return got.reshape(c.h, pitch)[:, : c.w * 2]


def _assert_exact(name, img, what=""):
    want = S.want_yu64(name)
    bad = img != want
    assert not bad.any(), "%s%s: %d of %d YU64 words differ from the oracle, first at (row, word) %s" % (name, what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))


def _assert_in_interval(name, img, what=""):
    lo, hi = S.want_yuy2_interval(name)
    ok = (img == lo) | (img == hi)
    assert ok.all(), "%s%s: %d of %d bytes are outside the oracle's dither interval, first at (row, byte) %s" % (name, what, (~ok).sum(), ok.size, tuple(np.argwhere(~ok)[0]))


@pytest.mark.parametrize("name", S.PROGRESSIVE + S.EXTRA)
def test_yu64_of_hand_made_samples_equals_oracle(name):
    """The dense-band output of k_dec_tiles, word for word."""
    _assert_exact(name, _yu64(name))


@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("name", ["full_tile", "mixed"])
def test_yu64_when_a_workgroup_decodes_tile_after_tile(name, grid):
    """CFHD_AMD_DX_GRID_TILES: k_dec_tiles with 1 and with 3 workgroups (read when a handle prepares its decoder), as in a batch with more tiles than the chip holds
    workgroups: the LDS image must be clear again when the next tile is decoded into it.  `full_tile`: tiles of the full DX_TILE, values at the end of one and zeros at
    the end of the next; `mixed`: dense tiles in front of empty ones."""
    os.environ["CFHD_AMD_DX_GRID_TILES"] = grid
    try:
        img = _yu64(name)
    finally:
        del os.environ["CFHD_AMD_DX_GRID_TILES"]
    _assert_exact(name, img, " with %s workgroups" % grid)


@pytest.mark.parametrize("name", REPAIR_CASES)
def test_yu64_of_hand_made_samples_without_speculation(name):
    """CFHD_AMD_DX_SPECULATE=0: every chunk but a band's first assumes a wrong start, so k_dec_chain, k_dec_repair and k_dec_reindex redo them all."""
    os.environ["CFHD_AMD_DX_SPECULATE"] = "0"
    try:
        img = _yu64(name)
    finally:
        del os.environ["CFHD_AMD_DX_SPECULATE"]
    _assert_exact(name, img, " without speculation")


@pytest.mark.parametrize("name", S.PROGRESSIVE + S.EXTRA)
def test_yuy2_of_hand_made_samples_block_lists_equal_dense_bands(name):
    """CFHD_AMD_INVERSE=strip: the level-1 bands leave k_dec_tiles as block lists with occupancy masks and k_inv_yuv422_strip_blocks gathers them; with
    CFHD_AMD_DEC_BLOCKS=0 the dense bands feed the same strip kernel.  Both pictures lie in the oracle's dither interval, and they are identical: the dither is the
    library's own hash of the position, so a block dropped from a list shows even inside the interval."""
    os.environ["CFHD_AMD_INVERSE"] = "strip"
    try:
        lists = _yuy2(name).copy()
        os.environ["CFHD_AMD_DEC_BLOCKS"] = "0"
        try:
            dense = _yuy2(name).copy()
        finally:
            del os.environ["CFHD_AMD_DEC_BLOCKS"]
    finally:
        del os.environ["CFHD_AMD_INVERSE"]
    _assert_in_interval(name, lists, " (block lists)")
    _assert_in_interval(name, dense, " (dense bands)")
    bad = lists != dense
    assert not bad.any(), "%s: block lists and dense bands give different pictures in %d bytes, first at %s" % (name, bad.sum(), tuple(np.argwhere(bad)[0]))


@pytest.mark.parametrize("route", ["default", "strip"])
def test_interlaced_peaks_sample_lies_in_the_oracle_interval(route):
    """The difference-coded band in code set 18 with a peak table and rows that are one run, to YUY2 under the default route and under CFHD_AMD_INVERSE=strip, against
    oracle_inverse_interlaced_yuv422 with dither 0 and 1.  The weaker witness: YU64 of an interlaced sample is refused at full resolution, so an error the 10 -> 8 bit
    shift swallows passes here; the pyramid itself is pinned on the emulated kernels (test_hand_made_samples.py)."""
    if route == "strip": os.environ["CFHD_AMD_INVERSE"] = "strip"
    try:
        img = _yuy2("interlaced_peaks")
    finally:
        os.environ.pop("CFHD_AMD_INVERSE", None)
    _assert_in_interval("interlaced_peaks", img, " (%s route)" % route)


def _gathered(pixfmt, handles=8, rounds=3):
    """`handles` threads, each with its own decoder handle, decode different cases at the same moment (the arrangement of
    test_concurrent_decoders_share_launches_and_stay_exact; all cases share one geometry): calls that overlap are gathered into one launch, whose chunk counter then runs
    over frames with bands of 1 to many chunks.  Thread t decodes case (t * (1, 3, 5)[r] + r) mod 8 in round r -- a permutation of the eight in every round, so no two
    handles decode the same case and a handle meets other neighbours each time; the threads start a round together."""
    names = list(S.PROGRESSIVE)
    assert len(names) == 8 and len({(S.case(n).w, S.case(n).h) for n in names}) == 1 and rounds <= 3
    L = product()
    for nm in names: S.want_yuy2_interval(nm) if pixfmt == PIX_YUY2 else S.want_yu64(nm)      # (computed before the threads start: one reference, shared, read-only)
    errors = []
    gate = threading.Barrier(handles)

    def worker(t):
        try:
            dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
            try:
                for r in range(rounds):
                    nm = names[(t * (1, 3, 5)[r] + r) % 8]
                    gate.wait(timeout=120)
                    if pixfmt == PIX_YUY2: _assert_in_interval(nm, _yuy2(nm, decoder=dec), " (thread %d, round %d)" % (t, r))
                    else: _assert_exact(nm, _yu64(nm, decoder=dec), " (thread %d, round %d)" % (t, r))
            finally:
                L.CFHD_CloseDecoder(dec)
        except BaseException as e:                                 # noqa: surfaced in the main thread
            errors.append(e); gate.abort()

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(handles)]
    for t in threads: t.start()
    for t in threads: t.join()
    real = [e for e in errors if not isinstance(e, threading.BrokenBarrierError)]
    if errors: raise (real or errors)[0]


@pytest.mark.parametrize("out", ["YU64", "YUY2"])
def test_gathered_launch_of_hand_made_samples(out):
    """Eight handles on eight threads, a different progressive case each (`mixed` and `one_run` among them), three rounds; YU64 exact, YUY2 inside the interval."""
    _gathered(fourcc(out))
