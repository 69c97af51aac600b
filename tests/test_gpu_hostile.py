"""Hostile pictures on the real kernels (run with `pytest -m gpu` on an MI355X; tests/test_product_emulated.py runs every case on the emulated product in the CPU suite).

The rest of the GPU suite feeds the kernels natural pictures.  Here: flat extremes (whole bands of zeros), noise on every byte (bands without a zero, saturating
arithmetic on the hardware's packed instructions), one-pixel stripes and checkerboards, single impulses (one listed block in an otherwise empty segment), edges on the
1984-pixel segment boundary of the strip kernels, and samples too large for the sample buffer (the entropy stage's overflow path).  Pictures: tests/hostile_pictures.py.

  encode: bytes equal the oracle's transform + the host writer (all of them, metadata taken from the sample) and, masked, the live reference encoder's
  decode: every byte in the oracle's dither interval (test_gpu_parity._check_decode, live reference leg included)
  the reference is only called on pictures that `legal_for_reference` admits: it overruns its own sample buffer on the others."""
import ctypes, os
import numpy as np
import pytest
from cfhd_testlib import *
import hostile_pictures as H
from test_gpu_parity import _check_decode, _batched_yuy2_round_trip_equals_reference, _batch_api, _reference_must_be_present      # noqa: F401 (the fixture applies here too)

pytestmark = pytest.mark.gpu
W, HT = 336, 252            # tiled kernels, pad rows 252 -> 256, odd lowpass widths
ERR_CODEC_ERROR = 2048      # CFHD_ERROR_CODEC_ERROR


def _want_sample(frame, w, h, quality, fmt, frame_number, sample):
    """Oracle transform + host writer of `frame`, with the metadata block of `sample` (GUID, date, time: the encoder's own)."""
    uyvy = int(fmt == "2vuy")
    plan = Plan(w, h, pixkind=PIXKIND[fmt], quality=quality)
    coeffs = oracle_forward_yuv422(plan, frame.reshape(-1), 2 * w, uyvy=uyvy)
    off, n = first_metadata_chunk(sample)
    return product_write_sample_host(plan, coeffs, frame_number, meta_global=sample[off:off + n], input_format=COLOR_FORMAT_UYVY if uyvy else COLOR_FORMAT_YUYV)


def _intra_case(name, quality, fmt):
    frame = H.yuy2(name, W, HT, fmt).reshape(-1)
    pixfmt = PIX_2VUY if fmt == "2vuy" else PIX_YUY2
    mine = amd_encode_frames([frame], 2 * W, W, HT, pixfmt, quality=quality)[0]
    want = _want_sample(frame, W, HT, quality, fmt, 1, mine)
    assert len(mine) == len(want), "%d bytes, oracle + host writer %d" % (len(mine), len(want))
    assert mine == want, "sample differs from the oracle + host writer at byte %d" % next(k for k in range(len(want)) if mine[k] != want[k])
    assert H.legal_for_reference(want, W, HT, 2), "%s at quality %d is not a legal case: %d bytes" % (name, quality, len(want))
    ref = ref_encode_frames([frame], 2 * W, W, HT, pixfmt, quality=quality)[0]
    assert mask_volatile_metadata(mine) == mask_volatile_metadata(ref), "sample differs from the live reference"
    _check_decode(mine, frame, W, HT, pixfmt, reference_psnr=_movable_bytes(mine, W, HT, fmt) > H.PSNR_WITNESS_MIN_MOVABLE)


def _movable_bytes(sample, w, h, fmt="YUY2"):
    """Bytes of the exact reconstruction that the dither bit can move (hostile_pictures.PSNR_WITNESS_MIN_MOVABLE)."""
    uyvy = int(fmt == "2vuy")
    plan = Plan(w, h, pixkind=PIXKIND[fmt])
    deq = oracle_decode_pyramid(sample, plan)
    return int((oracle_inverse_yuv422(plan, deq, 0, uyvy=uyvy)[:h] != oracle_inverse_yuv422(plan, deq, 1, uyvy=uyvy)[:h]).sum())


@pytest.mark.parametrize("name,quality", H.YUY2_CASES)
def test_intra_422_hostile_pictures_yuy2(name, quality):
    _intra_case(name, quality, "YUY2")


@pytest.mark.parametrize("name,quality", [c for c in H.YUY2_CASES if c[1] == 4])          # (the other byte order once: the FILMSCAN1 list)
def test_intra_422_hostile_pictures_2vuy(name, quality):
    _intra_case(name, quality, "2vuy")


class _env:
    def __init__(self, **kv): self.kv = kv
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.mark.parametrize("name", H.STRIP_CASES)
def test_strip_kernels_hostile_pictures_across_the_segment_boundary(name):
    """2048 x 72 through the batched path with the strip kernels forced: two segments, 1984 pixels and a partial one.  The picture beside an ordinary one (the batch holds
    two frames); block lists and dense level-1 bands must give the same pictures byte for byte."""
    w, h = H.STRIP_W, H.STRIP_H
    def frames_from(nuniq, w, h):
        frames = [H.yuy2(name, w, h).reshape(-1), synth_yuy2(w, h, 5)[0]][:nuniq]
        plan = Plan(w, h)
        for f in frames:                                    # legality before the reference sees a frame (the helper encodes all of them with one reference encoder)
            want = product_write_sample_host(plan, oracle_forward_yuv422(plan, f, 2 * w), 1)
            assert H.legal_for_reference(want, w, h, 2), "%s is not a legal case: %d bytes" % (name, len(want))
        return frames, 2 * w
    expect = {0: "k_fwd_yuv422_strip_blocks", 1: "k_fwd_plane_strip", 2: "k_fwd_plane_strip", 3: "k_inv_yuv422_strip_blocks", 4: "k_inv_plane_strip", 5: "k_inv_plane_strip"}
    with _env(CFHD_AMD_FORWARD="strip", CFHD_AMD_INVERSE="strip", CFHD_AMD_PLANES="strip"):
        lists = _batched_yuy2_round_trip_equals_reference(w, h, 2, 2, expect=expect, frames_from=frames_from)
        with _env(CFHD_AMD_DEC_BLOCKS="0"):
            dense = _batched_yuy2_round_trip_equals_reference(w, h, 2, 2, expect={**expect, 3: "k_inv_yuv422_strip"}, frames_from=frames_from)
    assert all(np.array_equal(a, b) for a, b in zip(lists, dense))


# ---- oversize samples: no reference call anywhere below

@pytest.mark.parametrize("entropy", ["gpu", "host"])
@pytest.mark.parametrize("name", H.OVERSIZE)
def test_oversize_sample_is_refused_and_the_handle_goes_on(name, entropy):
    """A frame whose sample does not fit the sample buffer: CFHD_EncodeSample returns CFHD_ERROR_CODEC_ERROR (k_ent_layout's overflow path: size 0, k_ent_emit leaves), and
    the next call on the same handle encodes an ordinary frame as frame number 2, byte for byte the oracle + host writer."""
    L = product()
    big = H.yuy2(name, W, HT).reshape(-1)
    plan = Plan(W, HT)
    predicted = product_write_sample_host(plan, oracle_forward_yuv422(plan, big, 2 * W), 1)
    assert len(predicted) > W * HT * 2 + 65536, "the case is not oversize: %d bytes" % len(predicted)
    good, _ = synth_yuy2(W, HT, 3)
    with _env(**({"CFHD_AMD_ENTROPY": "host"} if entropy == "host" else {})):
        enc = ctypes.c_void_p()
        assert L.CFHD_OpenEncoder(ctypes.byref(enc), None) == 0
        try:
            assert L.CFHD_PrepareToEncode(enc, W, HT, PIX_YUY2, ENCODED_YUV422, 0, QUALITY_FILMSCAN1) == 0
            rc = L.CFHD_EncodeSample(enc, big.ctypes.data_as(ctypes.c_void_p), 2 * W)
            assert rc == ERR_CODEC_ERROR, "CFHD_EncodeSample of an oversize frame -> %d (%s)" % (rc, amd_last_error())
            rc = L.CFHD_EncodeSample(enc, good.ctypes.data_as(ctypes.c_void_p), 2 * W)
            assert rc == 0, "the call behind it -> %d (%s)" % (rc, amd_last_error())
            p = ctypes.c_void_p(); n = ctypes.c_size_t()
            assert L.CFHD_GetSampleData(enc, ctypes.byref(p), ctypes.byref(n)) == 0
            sample = ctypes.string_at(p, n.value)
        finally:
            L.CFHD_CloseEncoder(enc)
    assert sample == _want_sample(good, W, HT, QUALITY_FILMSCAN1, "YUY2", 2, sample)


@pytest.mark.parametrize("entropy", ["gpu", "host", "host-handoff"])
@pytest.mark.parametrize("name", H.OVERSIZE)
def test_oversize_frame_in_a_batch_fails_the_pass_and_spares_its_neighbours(name, entropy):
    """cfhd_amd_batch_roundtrip promises "total sample bytes, or < 0" (include/cfhd_amd.h): a pass with an oversize frame between two ordinary ones returns < 0 -- and the
    samples of the two ordinary frames are there all the same, byte for byte the oracle + host writer with frame numbers 1 and 3."""
    L = _batch_api()
    frames = [synth_yuy2(W, HT, 3)[0], H.yuy2(name, W, HT).reshape(-1), synth_yuy2(W, HT, 4)[0]]
    with _env(**{"gpu": {}, "host": {"CFHD_AMD_ENTROPY": "host"}, "host-handoff": {"CFHD_AMD_HANDOFF": "host"}}[entropy]):
        b = L.cfhd_amd_batch_create(W, HT, PIX_YUY2, QUALITY_FILMSCAN1, 3, 4)
        assert b, amd_last_error()
        try:
            for i, f in enumerate(frames):
                assert L.cfhd_amd_batch_upload(b, i, f.ctypes.data_as(ctypes.c_void_p), 2 * W) == 0
            rc = L.cfhd_amd_batch_roundtrip(b)
            assert rc == -3, "a pass with an oversize frame -> %d" % rc                  # (cfhd_batch.cpp: -3 = a sample does not fit its buffer)
            for i in (0, 1, 2):
                p = ctypes.c_void_p(); sz = ctypes.c_size_t()
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                if i == 1: assert sz.value == 0, "the oversize frame reports %d bytes" % sz.value; continue
                assert sz.value > 0, "frame %d has no sample" % i
                sample = ctypes.string_at(p, sz.value)
                assert sample == _want_sample(frames[i], W, HT, QUALITY_FILMSCAN1, "YUY2", i + 1, sample), "frame %d" % i
            # the batch goes on: a pass of three ordinary frames behind the failed one (which did not count as a step: frame numbers 1..3 again), samples and pictures
            frames[1] = synth_yuy2(W, HT, 6)[0]
            assert L.cfhd_amd_batch_upload(b, 1, frames[1].ctypes.data_as(ctypes.c_void_p), 2 * W) == 0
            assert L.cfhd_amd_batch_roundtrip(b) > 0, amd_last_error()
            plan = Plan(W, HT)
            for i in range(3):
                p = ctypes.c_void_p(); sz = ctypes.c_size_t()
                assert L.cfhd_amd_batch_get_sample(b, i, ctypes.byref(p), ctypes.byref(sz)) == 0
                sample = ctypes.string_at(p, sz.value)
                assert sample == _want_sample(frames[i], W, HT, QUALITY_FILMSCAN1, "YUY2", i + 1, sample), "second pass, frame %d" % i
                out = np.zeros(HT * W * 2, np.uint8)
                assert L.cfhd_amd_batch_download_output(b, i, out.ctypes.data_as(ctypes.c_void_p), 2 * W) == 0
                deq = oracle_decode_pyramid(sample, plan)
                lo, hi = oracle_inverse_yuv422(plan, deq, 0)[:HT], oracle_inverse_yuv422(plan, deq, 1)[:HT]
                img = out.reshape(HT, 2 * W)
                assert ((img == lo) | (img == hi)).all(), "second pass, frame %d leaves the dither interval" % i
        finally:
            L.cfhd_amd_batch_destroy(b)


def test_decode_of_a_sample_larger_than_the_encoders_buffer():
    """The 244 328-byte sample of the noise picture (the reference encoder can emit it; here the host writer makes it into a buffer of its own): the product decodes it --
    size is no reason to refuse a sample -- into the oracle's dither interval."""
    frame = H.yuy2("noise", W, HT).reshape(-1)
    plan = Plan(W, HT)
    ordinary = amd_encode_frames([synth_yuy2(W, HT, 3)[0]], 2 * W, W, HT)[0]           # (for an encoder's metadata block: GUID, date, time)
    off, n = first_metadata_chunk(ordinary)
    sample = product_write_sample_host(plan, oracle_forward_yuv422(plan, frame, 2 * W), 1, meta_global=ordinary[off:off + n])
    assert len(sample) == 244328
    _check_decode(sample, frame, W, HT)


@pytest.mark.parametrize("name", ["vstripes", "hstripes", "checker"])
def test_half_resolution_decode_of_stripes_and_checkerboard(name):
    """Half-resolution decode (level-1 lowpass, SATURATE_8U(value >> 4), no dither) of the samples with the largest highpass bands: exact against the oracle, as
    test_gpu_parity.test_half_resolution_decode holds natural pictures."""
    frame = H.yuy2(name, W, HT).reshape(-1)
    sample = amd_encode_frames([frame], 2 * W, W, HT)[0]
    plan = Plan(W, HT)
    want = oracle_half_resolution(plan, oracle_decode_pyramid(sample, plan))
    out, pitch, aw, ah = amd_decode_sample(sample, resolution=2)
    assert (aw, ah, pitch) == (W // 2, HT // 2, W)
    assert np.array_equal(out.reshape(ah, pitch), want)
    def leg():
        rout, rpitch = ref_decode_sample(sample, W, HT, resolution=2)
        return np.array_equal(rout.reshape(-1, rpitch)[:, :W], want)
    reference_leg(leg, 3, "4:2:2 at half resolution")


# ---- one shape per other transform family, with the extreme pictures of that family (hostile_pictures.FAMILY_CASES); each comparison follows the family's own test

def _legal_then_reference(predicted, w, h, bpp, encode):
    assert H.legal_for_reference(predicted, w, h, bpp), "not a legal case: %d bytes predicted" % len(predicted)
    return encode()


@pytest.mark.parametrize("name", ["checker", "noise"])
def test_rg48_hostile_pictures(name):
    """RG48 -> RGB 4:4:4 at 320 x 240, FILMSCAN1 (the highest quality at which the full-range noise is legal: 298 388 of 460 800 bytes): 0 / 65535 checkerboard and noise
    on every word.  Encode byte-identical (oracle + host writer, live reference), decode word-exact against oracle_inverse_rgb48 (test_rg48_decode_equals_reference_exactly)."""
    w, h = 320, 240
    frame = H.words16(name, h, w, 3).reshape(-1).view(np.uint8).copy()
    plan = Plan(w, h, pixkind=PIXKIND["RG48"], enc=3)
    coeffs = oracle_forward_planes(plan, rg48_planes(frame, w * 6, w, h))
    mine = amd_encode_frames([frame], w * 6, w, h, PIX_RG48, encoded=ENCODED_RGB444)[0]
    off, n = first_metadata_chunk(mine)
    want = product_write_sample_host(plan, coeffs, 1, meta_global=mine[off:off + n], input_format=COLOR_FORMAT_RG48, color_space=0)
    assert mine == want
    ref = _legal_then_reference(want, w, h, 6, lambda: ref_encode_frames([frame], w * 6, w, h, PIX_RG48, encoded=ENCODED_RGB444)[0])
    assert len(mine) == len(ref) and mask_volatile_metadata(mine) == mask_volatile_metadata(ref)
    exact = oracle_inverse_rgb48(plan, oracle_decode_pyramid(mine, plan))[:h]
    got, gpitch, aw, ah = amd_decode_sample(mine, PIX_RG48)
    assert (aw, ah) == (w, h)
    a = np.frombuffer(got.tobytes(), np.uint16).reshape(h, gpitch // 2)[:, : w * 3]
    assert np.array_equal(a, exact), "%d words differ from the exact reconstruction" % (a != exact).sum()
    def leg():
        r, rp = ref_decode_sample(mine, w, h, PIX_RG48)
        return np.array_equal(np.frombuffer(r.tobytes(), np.uint16).reshape(h, rp // 2)[:, : w * 3], exact)
    reference_leg(leg, 3, "RGB 4:4:4 -> RG48")


def test_b64a_hostile_picture_with_alternating_alpha():
    """b64a -> RGBA 4:4:4:4 at 320 x 240: colour checkerboard 0 / 65535, alpha alternating 65535 / 0 from pixel to pixel (both ends of the companding curve, which leaves
    0 and 4095 alone).  As test_b64a_encode_bitstream_identical / test_b64a_decode_equals_reference."""
    w, h = 320, 240
    px = H.b64a_checker_alternating_alpha(w, h)
    frame = px.reshape(-1).view(np.uint8).copy()
    plan = Plan(w, h, pixkind=PIXKIND["b64a"], enc=ENC["4444"], quality=QUALITY_FILMSCAN1 | 0x20000000)
    coeffs = oracle_forward_planes(plan, b64a_planes(frame, w * 8, w, h))
    mine = amd_encode_frames([frame], w * 8, w, h, PIX_B64A, encoded=ENCODED_RGBA4444)[0]
    off, n = first_metadata_chunk(mine)
    want = product_write_sample_host(plan, coeffs, 1, meta_global=mine[off:off + n], input_format=COLOR_FORMAT_B64A, color_space=0)
    assert mine == want
    ref = _legal_then_reference(want, w, h, 8, lambda: ref_encode_frames([frame], w * 8, w, h, PIX_B64A, encoded=ENCODED_RGBA4444)[0])
    assert len(mine) == len(ref) and mask_volatile_metadata(mine) == mask_volatile_metadata(ref)
    dplan = Plan(w, h, pixkind=PIXKIND["b64a"], enc=ENC["4444"])
    pyramid = oracle_decode_pyramid(mine, dplan)
    exact = oracle_inverse_rgb48(dplan, pyramid, b64a=True)[:h]
    got, gpitch, aw, ah = amd_decode_sample(mine, PIX_B64A)
    assert (aw, ah, gpitch) == (w, h, w * 8)
    a = np.frombuffer(got.tobytes(), np.uint16).reshape(h, gpitch // 2)
    assert np.array_equal(a, exact), "%d words differ from the exact reconstruction" % (a != exact).sum()
    raw = oracle_inverse_rgb48(dplan, pyramid, b64a=False)[:h]
    def leg():
        r, rp = ref_decode_sample(mine, w, h, PIX_B64A)
        b = np.frombuffer(r.tobytes(), np.uint16).reshape(h, rp // 2)[:, : w * 4]
        colour = all(np.array_equal(b[:, k::4], exact[:, k::4]) for k in (1, 2, 3))
        rows = (b[:, 0::4] == exact[:, 0::4]).all(axis=1) | (b[:, 0::4] == raw[:, 3::4]).all(axis=1)
        return bool(colour and rows.all())
    reference_leg(leg, 3, "RGBA 4:4:4:4 -> b64a", racy=True)      # (the reference's alpha race, bayer.c:13871 / :16034)


def test_byr4_hostile_mosaic_between_both_clips():
    """BYR4 at 192 x 96, photosites alternating 65535 / 0 in both directions: red and blue at one clip, both greens at the other, so R-G and B-G sit at the ends of their
    range.  Encode as test_byr4_encode_bitstream_identical, decode as test_bayer_decode_to_byr4_equals_reference_exactly."""
    w, h = 192, 96
    mosaic = H.words16("checker", h, w, 1)
    frame = mosaic.reshape(-1).view(np.uint8).copy()
    plan = Plan(w, h, pixkind=PIXKIND["BYR4"], enc=ENC["bayer"])
    coeffs = oracle_forward_planes(plan, byr4_planes(mosaic))
    mine = amd_encode_frames([frame], w * 2, w, h, PIX_BYR4, encoded=ENCODED_BAYER)[0]
    off, n = first_metadata_chunk(mine)
    want = product_write_sample_host(plan, coeffs, 1, meta_global=mine[off:off + n], input_format=COLOR_FORMAT_BYR4, color_space=0)
    assert mine == want
    ref = _legal_then_reference(want, w, h, 2, lambda: ref_encode_frames([frame], w * 2, w, h, PIX_BYR4, encoded=ENCODED_BAYER)[0])
    assert len(mine) == len(ref) and mask_volatile_metadata(mine) == mask_volatile_metadata(ref)
    got, gpitch, aw, ah = amd_decode_sample(mine, PIX_BYR4)
    assert (aw, ah, gpitch) == (w, h, w * 2)
    a = np.frombuffer(got.tobytes(), np.uint16).reshape(h, gpitch // 2)[:, :w]
    exact = oracle_inverse_byr4(plan, oracle_decode_pyramid(mine, plan))[:h, :w]
    assert np.array_equal(a, exact), "%d words differ from the exact reconstruction" % (a != exact).sum()
    def leg():
        r, rp = ref_decode_sample(mine, w, h, PIX_BYR4)
        img = np.frombuffer(r.tobytes(), np.uint16).reshape(h, rp // 2)[:, :w]
        return np.array_equal(img, a) or "%d words differ" % (img != a).sum()
    reference_leg(leg, 6, "Bayer -> BYR4")


@pytest.mark.parametrize("picture,peaks", [("hstripes", False), ("flicker", True)])
def test_interlaced_rows_255_and_0_on_the_device_entropy_route(picture, peaks):
    """Interlaced YUY2 at 320 x 64, luma rows 255 / 0: the two fields are a full range apart, the largest field difference there is.  The expectations of
    test_interlaced_encode_peak_table_frames: the device entropy stage alone writes the sample (CFHD_AMD_ENTROPY=device), bytes equal the reference's, decode in the
    dither interval of the interlaced inverse (_check_decode).  Measured on the reference: with flat fields ("hstripes") the difference-coded band is zero behind its
    first column and the sample (4 596 bytes) carries NO peak table; the same rows with the fields exchanged every 37 pixels (cfhd_testlib.field_flicker_frame) carry one.
    Both are held to what the reference writes."""
    w, h = 320, 64
    frame = H.yuy2("hstripes", w, h).reshape(-1) if picture == "hstripes" else field_flicker_frame(w, h)[0]
    plan = Plan(w, h, progressive=0)
    coeffs = oracle_forward_interlaced_yuv422(plan, frame, 2 * w)
    with _env(CFHD_AMD_ENTROPY="device"):                      # (a sample handed to the host writer fails the call)
        mine = amd_encode_frames([frame], 2 * w, w, h, PIX_YUY2, flags=1)[0]
    off, n = first_metadata_chunk(mine)
    want = product_write_sample_host(plan, coeffs, 1, meta_global=mine[off:off + n], progressive=0)
    assert mine == want
    ref = _legal_then_reference(want, w, h, 2, lambda: ref_encode_frames([frame], 2 * w, w, h, PIX_YUY2, flags=1)[0])
    assert len(mine) == len(ref) and mask_volatile_metadata(mine) == mask_volatile_metadata(ref)
    tables = sum(1 for i in range(0, len(ref) - 12, 4) if ref[i:i + 2] == b"\xff\xb5" and ref[i + 4:i + 6] == b"\xff\xb4" and ref[i + 8:i + 10] == b"\xff\xb6" and ref[i + 10:i + 12] != b"\0\0")
    assert (tables > 0) == peaks, "%d bands of the sample have a peak table" % tables
    _check_decode(mine, frame, w, h, PIX_YUY2, interlaced=True, reference_psnr=False)      # (flat fields: nothing for the dither to move, hostile_pictures.PSNR_WITNESS_MIN_MOVABLE)


@pytest.mark.parametrize("first,second", [("flat0", "flat255"), ("flat255", "flat0")])
def test_two_frame_group_of_flat_0_and_flat_255(first, second):
    """A two-frame group at 320 x 240 whose frames are flat 0 and flat 255 (every byte, chroma too), in both orders: the temporal highpass is the full range in every
    coefficient and saturates.  Encode as test_gop_encode_bitstream_identical (plus the oracle + host writer), decode as test_gop_decode_reference_samples."""
    w, h = 320, 240
    frames = [H.yuy2(first, w, h).reshape(-1), H.yuy2(second, w, h).reshape(-1)]
    gp = GopPlan(w, h)
    coeffs = oracle_forward_gop(gp, frames[0], frames[1], 2 * w)
    mine = amd_encode_frames(frames, 2 * w, w, h, PIX_YUY2, flags=ENCODING_FLAGS_2FRAME_GOP)
    off, n = first_metadata_chunk(mine[1])
    want = product_write_gop_host(gp, 0, coeffs, 1, meta_global=mine[1][off:off + n])
    assert mine[1] == want
    refs = _legal_then_reference(want, w, h, 2, lambda: ref_encode_frames(frames, 2 * w, w, h, flags=ENCODING_FLAGS_2FRAME_GOP))
    assert [len(s) for s in mine] == [len(s) for s in refs]
    for i, (a, b) in enumerate(zip(mine, refs)): assert mask_volatile_metadata(a) == mask_volatile_metadata(b), "sample %d differs from the reference" % i
    # decode: the group, then the P-frame header behind it (a third call of the encoder writes it)
    samples = amd_encode_frames(frames + [frames[0]], 2 * w, w, h, PIX_YUY2, flags=ENCODING_FLAGS_2FRAME_GOP)
    L = product()
    dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
    aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
    sb = ctypes.create_string_buffer(samples[0], len(samples[0]))
    assert L.CFHD_PrepareToDecode(dec, 0, 0, PIX_YUY2, 1, 0, sb, len(samples[0]), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af)) == 0
    outs = []
    for s in samples:
        sb = ctypes.create_string_buffer(s, len(s)); out = np.full(w * 2 * ah.value, 7, np.uint8)
        assert L.CFHD_DecodeSample(dec, sb, len(s), out.ctypes.data_as(ctypes.c_void_p), w * 2) == 0, amd_last_error()
        outs.append(out.reshape(ah.value, w * 2))
    L.CFHD_CloseDecoder(dec)
    co = oracle_decode_group(samples[1], gp)
    lo, hi = oracle_inverse_gop(gp, co, 0), oracle_inverse_gop(gp, co, 1)
    for f in range(2):
        img = outs[1 + f][:h]
        ok = (img == lo[f][:h]) | (img == hi[f][:h])
        assert ok.all(), "frame %d: %d bytes outside the dither interval" % (f, (~ok).sum())
        assert psnr_yuy2(img, frames[f].reshape(h, w * 2)) > 38.0
    def leg():
        got = ref_decode_group_frames(samples, w, h, PIX_YUY2)
        for f in range(2):
            r = got[0][f]
            if r is not None and not ((r == lo[f][:h]) | (r == hi[f][:h])).all(): return "frame %d: the reference decoder's picture leaves the interval" % f
        return True
    reference_leg(leg, 2, "two-frame groups -> 8-bit 4:2:2 (interval only)")


def test_decode_of_a_sample_that_saturates_the_inverse_transform():
    """No encoder emits it: every sample an encoder writes keeps the sums of the inverse transform below half the int16 range (four times the 10- or 12-bit source range),
    so no picture, however hostile, reaches the clamp of the packed saturating adds (v_pk_add_i16 / v_pk_sub_i16 with clamp) on the decode side.  A sample with full-size
    highpass bands at levels 2 and 3 does: the host writer makes it from a hand-made pyramid (+-30 000 after dequantization in every highpass coefficient of those
    levels, the lowpass band of a mid-grey picture).  The product decodes it into the dither interval of the oracle's inverse, whose 16-bit sums saturate as the
    reference's SSE2 code does.  No reference call."""
    rng = np.random.default_rng(8)
    plan = Plan(W, HT)
    coeffs = oracle_forward_yuv422(plan, H.yuy2("flat128", W, HT).reshape(-1), 2 * W)
    for c in range(3):
        for lv in (1, 2):
            for b in (1, 2, 3):
                d = plan.band[(c, lv, b)]
                v = plan.view(coeffs, c, lv, b)
                v[:, : d["width"]] = rng.choice(np.array([-1, 1], np.int16), (d["height"], d["width"])) * np.int16(30000 // d["quant"])
    sample = product_write_sample_host(plan, coeffs, 1)
    out, pitch, aw, ah = amd_decode_sample(sample)
    img = out.reshape(ah, pitch)[:, : 2 * W]
    deq = oracle_decode_pyramid(sample, plan)
    lo, hi = oracle_inverse_yuv422(plan, deq, 0)[:HT], oracle_inverse_yuv422(plan, deq, 1)[:HT]
    assert (lo == 0).mean() > 0.1 and (lo == 255).mean() > 0.1, "the sample does not drive the picture into both clips"
    ok = (img == lo) | (img == hi)
    assert ok.all(), "%d of %d bytes are outside the dither interval" % ((~ok).sum(), ok.size)
