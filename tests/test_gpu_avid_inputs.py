"""The five Avid 4:2:2 encoder inputs (avu8, av16, a106, a214, av28) on the GPU: CFHD_EncodeSample, two-frame groups, the encoder pool and encode-only batches give
the live reference encoder's samples byte for byte (level 1 through the loaders of k_fwd_packed16 / k_fwd_gop_packed16), and the samples -- ordinary 4:2:2 samples --
decode to YU64 no further from the picture than the reference decoder leaves the reference's own sample.

Measured round-trip tolerance (the largest luma error, in 16-bit YU64 units, of the reference decoder on the reference's sample against the planes << 6; printed per
case by test_round_trip_to_yu64), on an MI355X: 832 to 1216 for avu8 / av16 / a106 / av28, 1216 to 1664 for a214 (whose top rows are noise over the whole int16
range); the product's error equalled the reference's in all twenty cases.  Frames: tests/avid_frames.py."""
import ctypes, struct
import numpy as np
import pytest
import cfhd_testlib as T
import avid_frames as A

pytestmark = pytest.mark.gpu
GOP = T.ENCODING_FLAGS_2FRAME_GOP
SIZES = [(192, 96), (208, 104)]      # one luma tile per tile row / a second one of 8 of 64 columns (4 in the chroma planes)
_intra = {}


def _intra_samples(name, w, h):
    """(product's samples, reference's samples, planes) of two frames, encoded once and shared."""
    key = (name, w, h)
    if key not in _intra:
        assert T.have_ref(), "oracle/_ref/libcfhd_ref.so is missing"
        data, pitch, planes = A.frames(name, w, h, 2)
        mine = T.amd_encode_frames(data, pitch, w, h, A.FOURCC[name])
        refs = T.ref_encode_frames(data, pitch, w, h, pixfmt=A.FOURCC[name])
        _intra[key] = (mine, refs, planes)
    return _intra[key]


def _same(mine, refs):
    assert [len(s) for s in mine] == [len(s) for s in refs]
    for i, (a, b) in enumerate(zip(mine, refs)):
        assert T.mask_volatile_metadata(a) == T.mask_volatile_metadata(b), "sample %d differs from the reference" % i


def _without_frame_counters(sample):
    """The frame number (optional tag 69) and the UFRM counter count per encoder: zeroed between encoders with different histories (tests/test_gpu_parity.py)."""
    b = bytearray(T.mask_volatile_metadata(sample))
    k = bytes(b[:160]).find(struct.pack(">h", -69))
    if k >= 0: b[k + 2:k + 4] = b"\0\0"
    u = bytes(b[:1024]).find(b"UFRM")
    if u >= 0: b[u + 8:u + 12] = b"\0\0\0\0"
    return bytes(b)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", A.LAYOUTS)
def test_intra_samples_equal_the_reference(name, w, h):
    mine, refs, _ = _intra_samples(name, w, h)
    _same(mine, refs)
    assert mine[0] != mine[1]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", A.LAYOUTS)
def test_group_stream_equals_the_reference(name, w, h):
    data, pitch, _ = A.frames(name, w, h, 4)
    mine = T.amd_encode_frames(data, pitch, w, h, A.FOURCC[name], flags=GOP)
    _same(mine, T.ref_encode_frames(data, pitch, w, h, pixfmt=A.FOURCC[name], flags=GOP))
    assert len(mine[0]) == 40 and len(mine[2]) == 24 and mine[1] != mine[3]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", A.LAYOUTS)
def test_encoder_pool_keeps_order_and_bytes(name, w, h):
    """Two workers, six frames: the samples come back in submission order and equal the reference encoder's (frame counters apart: they count per worker)."""
    L = T.product()
    data, pitch, _ = A.frames(name, w, h, 6)
    refs = T.ref_encode_frames(data, pitch, w, h, pixfmt=A.FOURCC[name])
    pool = ctypes.c_void_p()
    assert L.CFHD_CreateEncoderPool(ctypes.byref(pool), 2, 6, None) == 0
    assert L.CFHD_PrepareEncoderPool(pool, w, h, A.FOURCC[name], T.ENCODED_YUV422, 0, T.QUALITY_FILMSCAN1) == 0
    assert L.CFHD_StartEncoderPool(pool) == 0
    for i, f in enumerate(data): assert L.CFHD_EncodeAsyncSample(pool, 100 + i, f.ctypes.data_as(ctypes.c_void_p), pitch, None) == 0
    got = []
    for _ in data:
        num = ctypes.c_uint32(); sb = ctypes.c_void_p()
        assert L.CFHD_WaitForSample(pool, ctypes.byref(num), ctypes.byref(sb)) == 0, T.amd_last_error()
        p = ctypes.c_void_p(); n = ctypes.c_size_t()
        assert L.CFHD_GetEncodedSample(sb, ctypes.byref(p), ctypes.byref(n)) == 0
        got.append((num.value, ctypes.string_at(p, n.value)))
        assert L.CFHD_ReleaseSampleBuffer(pool, sb) == 0
    assert L.CFHD_ReleaseEncoderPool(pool) == 0
    assert [n for n, _ in got] == [100 + i for i in range(len(data))]
    for i, (_, s) in enumerate(got): assert _without_frame_counters(s) == _without_frame_counters(refs[i]), "pool sample %d" % i


def _batch_api():
    L = T.product()
    L.cfhd_amd_batch_create_ex.restype = ctypes.c_void_p
    L.cfhd_amd_batch_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.cfhd_amd_batch_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    L.cfhd_amd_batch_roundtrip.restype = ctypes.c_longlong; L.cfhd_amd_batch_roundtrip.argtypes = [ctypes.c_void_p]
    L.cfhd_amd_batch_submit_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    L.cfhd_amd_batch_wait.restype = ctypes.c_longlong; L.cfhd_amd_batch_wait.argtypes = [ctypes.c_void_p]
    L.cfhd_amd_batch_kernel_name.restype = ctypes.c_char_p; L.cfhd_amd_batch_kernel_name.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.cfhd_amd_batch_get_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    L.cfhd_amd_batch_destroy.argtypes = [ctypes.c_void_p]
    return L


def _batch_samples(L, b, n):
    out = []
    for i in range(n):
        p = ctypes.c_void_p(); sz = ctypes.c_size_t()
        assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
        out.append(ctypes.string_at(p, sz.value))
    return out


@pytest.mark.parametrize("name", A.LAYOUTS)
def test_batch_mode_1_equals_the_synchronous_encoder(name):
    """Eight frames, encode only: uploaded one by one, then the same frames back to back from host memory (cfhd_amd_batch_submit_host); mode 0 is not created."""
    w, h, n = 192, 96, 8
    L = _batch_api()
    data, pitch, _ = A.frames(name, w, h, n)
    sync = [_without_frame_counters(s) for s in T.amd_encode_frames(data, pitch, w, h, A.FOURCC[name])]
    assert not L.cfhd_amd_batch_create_ex(w, h, A.FOURCC[name], T.ENCODED_YUV422, 0, T.QUALITY_FILMSCAN1, n, 1, 0)
    b = L.cfhd_amd_batch_create_ex(w, h, A.FOURCC[name], T.ENCODED_YUV422, 0, T.QUALITY_FILMSCAN1, n, 1, 1)
    assert b, T.amd_last_error()
    try:
        assert L.cfhd_amd_batch_kernel_name(b, 0) == b"k_fwd_packed16"
        for i, f in enumerate(data): assert L.cfhd_amd_batch_upload(b, i, f.ctypes.data_as(ctypes.c_void_p), pitch) == 0
        assert L.cfhd_amd_batch_roundtrip(b) > 0, T.amd_last_error()
        assert [_without_frame_counters(s) for s in _batch_samples(L, b, n)] == sync
        block = np.concatenate([np.asarray(f) for f in data[::-1]])      # the frames in reverse order, back to back
        assert L.cfhd_amd_batch_submit_host(b, block.ctypes.data_as(ctypes.c_void_p), data[0].size, pitch, None, 0, 0) == 0, T.amd_last_error()
        assert L.cfhd_amd_batch_wait(b) > 0, T.amd_last_error()
        assert [_without_frame_counters(s) for s in _batch_samples(L, b, n)] == sync[::-1]
    finally:
        L.cfhd_amd_batch_destroy(b)


def test_one_1080p_a214_frame():
    """1920 x 1080: the only geometry here whose tile grid has interior tiles and both edges in both directions, and a height that is no multiple of 8 -- the loader
    writes zeros below row 1079 and reads nothing there.  The reference reads eight rows past the frame, so it is handed a copy with eight more rows of -32768, the
    words its arithmetic clamps to 0 in every plane."""
    w, h = 1920, 1080
    data, pitch, _ = A.frames("a214", w, h, 1)
    mine = T.amd_encode_frames(data, pitch, w, h, A.FOURCC["a214"])
    padded = np.concatenate([np.asarray(data[0]), np.full(8 * 2 * w, -32768, np.int16).view(np.uint8)])
    _same(mine, T.ref_encode_frames([padded], pitch, w, h, pixfmt=A.FOURCC["a214"]))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", A.LAYOUTS)
def test_round_trip_to_yu64(name, w, h):
    """The product decodes its sample to YU64; luma lies within the quantizer's error of the planes the frame was made of.  The tolerance is measured, with no
    margin: the largest luma error the reference decoder leaves on the reference's own sample of the same frame -- both decode the same coefficients."""
    mine, refs, planes = _intra_samples(name, w, h)
    for i in range(2):
        want = planes[i][0].astype(np.int32) << 6
        out, pitch = T.ref_decode_sample(refs[i], w, h, T.PIX_YU64)
        tolerance = int(np.abs(out.view(np.uint16).reshape(h, pitch // 2)[:, : 2 * w : 2].astype(np.int32) - want).max())
        out, pitch, aw, ah = T.amd_decode_sample(mine[i], T.PIX_YU64)
        assert (aw, ah) == (w, h)
        err = int(np.abs(out.view(np.uint16).reshape(ah, pitch // 2)[:, : 2 * w : 2].astype(np.int32) - want).max())
        print("round trip %s %dx%d frame %d: reference decoder's largest luma error %d, product's %d (16-bit units)" % (name, w, h, i, tolerance, err))
        assert 0 < tolerance < 4096 and err <= tolerance
