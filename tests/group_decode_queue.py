"""The decode queue for streams of two-frame groups (cfhd_amd_decode_batch_create_groups: group samples of any encoder and the P-frame samples behind them, parsed
and decoded on the GPU): the helpers and test bodies shared by tests/test_gpu_group_decode_queue.py (hardware) and tests/test_group_decode_queue_emulated.py (the
same functions inside cfhd_testlib.emulated_product()).

The yardstick throughout is ONE CFHD_DecodeSample handle of this library, prepared on the first group sample and fed the same samples in the same order
(decode_queue.handle_pictures): its return codes are the queue's statuses, its pictures the queue's -- byte for byte for the outputs without dither, within the one
dither step for the full-resolution 8-bit outputs.  What the handle's pictures of groups are worth is pinned on the reference's group decoder by
tests/test_group_outputs_model_vs_ref.py.  The queue judges every pair alone; every case here keeps group samples in even entries, where "alone" and "one handle in
order" agree.
Test infrastructure only."""
import ctypes, os
import numpy as np
from cfhd_testlib import *
import decode_queue as DQ
from decode_queue import Queue, pack, scattered_blob, DeviceBlob, damaged, handle_pictures, walk_bands, device_copy, FOURCCS, FULL, HALF, QUARTER, V, SZ, VERDICT_KINDS, _sizes, _same

GOP = ENCODING_FLAGS_2FRAME_GOP
SOURCES = ("ref", "amd")
# (interlaced, w, h, output, resolution): no dither -- every picture equals the handle's byte for byte.  336 x 252: a coded height of 256, odd chroma lowpass widths;
# 384: whole 48-pixel groups of v210
EXACT_CASES = [(0, 320, 240, "YU64", FULL), (0, 336, 252, "RG48", FULL), (0, 384, 96, "v210", FULL), (0, 320, 240, "YUY2", HALF), (0, 320, 240, "b64a", HALF),
               (1, 320, 240, "RG48", FULL), (1, 320, 240, "YUY2", HALF)]
# (interlaced, w, h, dithered output, the exact output of the same samples)
DITHER_CASES = [(0, 320, 240, "YUY2", "YU64"), (0, 320, 240, "BGRA", "YU64"), (1, 320, 240, "YUY2", "RG48")]
# (8-bit RGB input, w, h): subband 7 of such groups is divided and coded in two passes.  The second geometry is the one whose luma first pass is longer than the
# kernel's 8 KB sequence: check_two_pass_on_the_device asserts it on the sample, and 640 x 480 is the first size tried at which it holds
TWO_PASS_CASES = [("RG24", 320, 240), ("BGRA", 320, 240), ("RG24", 640, 480)]
FOLLOWER_KINDS = ("first tag", "two bytes", "size 0")


def lib():
    L = DQ.lib()
    if not getattr(L, "_group_decode_queue_declared", False):
        L.cfhd_amd_decode_batch_create_groups.restype = V
        L.cfhd_amd_decode_batch_create_groups.argtypes = [V, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
        L._group_decode_queue_declared = True
    return L


class GroupQueue(Queue):
    """One decode batch of `ngroups` two-frame groups prepared on the group sample `first`: 2 * ngroups samples and pictures a pass."""
    def __init__(self, first, out, resolution, ngroups):
        self.L = lib(); self.n = 2 * ngroups
        fb = ctypes.create_string_buffer(first, len(first))
        self.b = self.L.cfhd_amd_decode_batch_create_groups(fb, len(first), FOURCCS[out], resolution, ngroups)
        assert self.b, "cfhd_amd_decode_batch_create_groups -> NULL (%s)" % amd_last_error()
        w = ctypes.c_int(); h = ctypes.c_int(); rb = ctypes.c_int()
        assert self.L.cfhd_amd_decode_batch_geometry(self.b, ctypes.byref(w), ctypes.byref(h), ctypes.byref(rb)) == 0
        self.w, self.h, self.row_bytes = w.value, h.value, rb.value


_streams = {}


def _rgb8_frames(name, w, h, n, static=False):
    """n frames of an 8-bit RGB input: frame 2 g + 1 is the complement of frame 2 g (the temporal highpass band then carries values of more than eight bits, so the
    second pass of subband 7 has something to code); static: every frame the same picture (the second pass is an all-zero band)."""
    px = 3 if name == "RG24" else 4
    out = []
    for g in range(n // 2):
        rng = np.random.default_rng(900 + (0 if static else g))
        y, x = np.mgrid[0:h, 0:w]
        f = np.zeros((h, w, px), np.uint8)
        for c in range(3):
            v = 128 + 100 * np.sin(x / (17.0 + 5 * c) + g) * np.cos(y / (13.0 + 3 * c)) + rng.normal(0, 12, (h, w))
            f[:, :, c] = np.clip(v, 0, 255).astype(np.uint8)
        if px == 4: f[:, :, 3] = 255
        second = f if static else 255 - f
        if px == 4 and not static: second[:, :, 3] = 255
        out += [np.ascontiguousarray(f).reshape(-1), np.ascontiguousarray(second).reshape(-1)]
    return out, w * px


def group_stream(source, w, h, interlaced=0, quality=QUALITY_FILMSCAN1, pix="YUY2", static=False):
    """The 8 samples -- group, P-frame sample, group, ... -- of 8 distinct frames = 4 groups from the reference's encoder ("ref") or the product's ("amd"), the 40-byte
    sequence header dropped; encoded once, shared, read-only.  (The encoder hands out a sample per call and the last P-frame sample with the call behind the last
    frame: one more frame is fed and its sample left out.)"""
    key = (source, w, h, interlaced, quality, pix, static, bool(DQ.use_emulated()))
    if key not in _streams:
        if pix == "YUY2": frames, pitch = [np.ascontiguousarray(DQ._yuy2_frame(w, h, i, bool(interlaced))) for i in range(8)], w * 2
        else: frames, pitch = _rgb8_frames(pix, w, h, 8, static)
        encode = ref_encode_frames if source == "ref" else amd_encode_frames
        stream = encode(frames + [frames[0]], pitch, w, h, FOURCCS[pix], ENCODED_YUV422, quality, GOP | (1 if interlaced else 0))
        assert len(stream) == 9 and len(stream[0]) == 40, [len(s) for s in stream]
        samples = stream[1:]
        assert all(len(s) == 24 for s in samples[1::2]) and all(s[:4] == b"\x00\x01\x00\x02" for s in samples[0::2])
        _streams[key] = samples
    return _streams[key]


# ---- 1. foreign groups
def check_foreign_exact(interlaced, w, h, out, resolution, source, samples=None):
    samples = samples if samples is not None else group_stream(source, w, h, interlaced)
    assert len(set(samples[0::2])) == 4 and len(samples) == 8
    want, geometry = handle_pictures(samples, out, resolution)
    q = GroupQueue(samples[0], out, resolution, 4)
    try:
        assert (q.w, q.h, q.row_bytes) == geometry
        ret, status, pictures = q.decode(samples)
        assert ret == 8 and status == [0] * 8, (ret, status, amd_last_error())
        for i in range(8):
            assert want[i][0] == 0
            _same(pictures[i], want[i][1], "%s -> %s sample %d" % ("interlaced" if interlaced else "progressive", out, i))
    finally:
        q.close()


# ---- 2. dithered
def check_foreign_dithered(interlaced, w, h, out, exact_out, source):
    samples = group_stream(source, w, h, interlaced)
    want, geometry = handle_pictures(samples, out, FULL)
    q = GroupQueue(samples[0], out, FULL, 4)
    try:
        assert (q.w, q.h, q.row_bytes) == geometry
        for step in range(2):                                    # (the seed follows the pass number: both passes stay inside the step)
            ret, status, pictures = q.decode(samples)
            assert ret == 8 and status == [0] * 8, (ret, status, amd_last_error())
            for i in range(8):
                d = np.abs(pictures[i].astype(np.int16) - want[i][1].astype(np.int16))
                assert d.max() <= 1, "%s pass %d sample %d: %d bytes further than one step from the handle's" % (out, step, i, int((d > 1).sum()))
    finally:
        q.close()
    check_foreign_exact(interlaced, w, h, exact_out, FULL, source)


# ---- 3. the band coded in two passes
def group_bands(sample):
    """[(wavelet number, band, BAND_ENCODING, position behind the band header, end of the payload)] of every band header of the group sample, in stream order, by the
    tag walk of walk_bands."""
    d = sample; pos = 0; pending_at = pending = 0; wavelet = band = encoding = 0; out = []
    while pos + 4 <= len(d):
        tag = int.from_bytes(d[pos: pos + 2], "big", signed=True); value = int.from_bytes(d[pos + 2: pos + 4], "big")
        tag = -tag if tag < 0 else tag
        pos += 4
        if tag & 0x4000:
            pos += 4 * ((((tag & 0xff) << 16) | value) if tag & 0x2000 else value); continue
        if tag & 0x2000:
            if (tag & 0xff00) == 0x2000: pending = 4 * (((tag & 0xff) << 16) | value); pending_at = pos
            continue
        if tag == 2: pos += 4 * value
        elif tag == 38: wavelet = value
        elif tag == 48: band = value; encoding = 3
        elif tag == 52: encoding = value
        elif tag == 4 and value == 0x0f0f: pos = pending_at + pending
        elif tag == 55:
            end = pending_at + pending
            out.append((wavelet, band, encoding, pos, end - 4)); pos = end
    return out


def two_pass_bands(sample):
    """[(bytes of pass 1 up to the BAND_SECONDPASS tag, bytes behind the tag)] of every band of the group sample that is coded in two passes (BAND_ENCODING 5), in
    channel order.  The tag is the one longword-aligned 00 52 00 00 of the payload."""
    out = []
    for wavelet, band, encoding, lo, hi in group_bands(sample):
        if encoding != 5: continue
        assert (wavelet, band) == (4, 0), "a two-pass band that is not subband 7"
        payload = sample[lo: hi]
        tags = [at for at in range(0, len(payload) - 3, 4) if payload[at: at + 4] == b"\x00\x52\x00\x00"]
        assert len(tags) == 1, tags
        out.append((tags[0], len(payload) - tags[0] - 4))
    return out


def check_two_pass_on_the_device(pix, w, h, source):
    samples = group_stream(source, w, h, pix=pix)
    still = group_stream(source, w, h, pix=pix, static=True)
    for g in range(4):
        bands, zero = two_pass_bands(samples[2 * g]), two_pass_bands(still[2 * g])
        assert len(bands) == len(zero) == 3, "subband 7 of every channel is coded in two passes"
        for c in range(3):
            assert bands[c][1] > zero[c][1], "group %d channel %d: the second pass carries nothing (%d bytes, an all-zero band's: %d)" % (g, c, bands[c][1], zero[c][1])
        # the large case: luma's first pass does not fit the kernel's 8 KB sequence, the carry between sequences runs
        if w >= 640: assert bands[0][0] > 8192, "group %d: luma's first pass is %d bytes" % (g, bands[0][0])
    check_foreign_exact(0, w, h, "YU64", FULL, source, samples=samples)


# ---- 4. mixed passes
def check_mixed_qualities(source):
    """FILMSCAN1 groups and groups of a rate-feedback quality (FILMSCAN2: the tables move from group to group) alternate in one pass."""
    w, h = 320, 240
    a, b = group_stream(source, w, h), group_stream(source, w, h, quality=5)
    assert len(set(len(s) for s in b[0::2])) > 1
    samples = a[0:2] + b[2:4] + a[4:6] + b[6:8]
    _check_against_the_handle(samples, "YU64")


def check_mixed_band_kinds(source):
    """Groups whose subband 7 is raw words (a YUY2 source) and groups whose subband 7 is coded in two passes (an RG24 source) of one geometry in one pass."""
    w, h = 320, 240
    a, b = group_stream(source, w, h), group_stream(source, w, h, pix="RG24")
    assert not two_pass_bands(a[0]) and len(two_pass_bands(b[0])) == 3
    _check_against_the_handle(a[0:2] + b[2:4] + b[4:6] + a[6:8], "YU64")
    _check_against_the_handle(b[0:2] + a[2:4] + a[4:6] + b[6:8], "YU64")


def _check_against_the_handle(samples, out):
    want, _ = handle_pictures(samples, out, FULL)
    q = GroupQueue(samples[0], out, FULL, 4)
    try:
        ret, status, pictures = q.decode(samples)
        assert status == [rc for rc, _ in want] == [0] * 8 and ret == 8, (ret, status)
        for i in range(8): _same(pictures[i], want[i][1], "mixed pass, sample %d" % i)
    finally:
        q.close()


# ---- 5. ingest
def check_ingest(source="ref"):
    """Plain memory, a registered blob and device memory: the samples scattered with gaps at odd byte offsets, no follower next to its group."""
    w, h, out = 320, 240, "YU64"
    samples = group_stream(source, w, h)
    want, _ = handle_pictures(samples, out, FULL)
    blob, offsets, sizes = scattered_blob(samples)
    for g in range(4): assert offsets[2 * g + 1] != offsets[2 * g] + sizes[2 * g], "follower %d lies behind its group" % g
    L = lib()
    q = GroupQueue(samples[0], out, FULL, 4)
    try:
        row, frame = q.row_bytes, q.row_bytes * q.h
        pics = np.full(frame * 8, 9, np.uint8)
        assert q.submit(blob, offsets, sizes, pics, frame, row) == 0, amd_last_error()
        assert q.wait(8) == (8, [0] * 8)
        for i in range(8): _same(pics[i * frame: (i + 1) * frame], want[i][1], "plain memory, sample %d" % i)
        pics2 = np.full(frame * 8, 9, np.uint8)
        assert L.cfhd_amd_register_host_buffer(blob.ctypes.data_as(V), blob.nbytes) == 0 and L.cfhd_amd_register_host_buffer(pics2.ctypes.data_as(V), pics2.nbytes) == 0
        try:
            assert q.submit(blob, offsets, sizes, pics2, frame, row) == 0, amd_last_error()
            assert q.wait(8) == (8, [0] * 8)
        finally:
            L.cfhd_amd_unregister_host_buffer(blob.ctypes.data_as(V)); L.cfhd_amd_unregister_host_buffer(pics2.ctypes.data_as(V))
        assert np.array_equal(pics2, pics), "registered memory and plain memory give different pictures"
        owner, dptr = device_copy(blob)
        if dptr is None: dptr = owner.ptr
        assert L.cfhd_amd_decode_batch_submit_device(q.b, dptr, blob.nbytes, _sizes(offsets), _sizes(sizes), 8) == 0, amd_last_error()
        assert q.wait(8) == (8, [0] * 8)
        for i, p in enumerate(q.pictures(8)): _same(p, pics[i * frame: (i + 1) * frame], "device memory, sample %d" % i)
        del owner
    finally:
        q.close()


# ---- 6. a short pass
def check_short_pass(source="ref"):
    """ngroups 4: a pass of 4 groups, then a pass of 1 group -- pictures 2 .. 7 of download_output are still the first pass's, and a picture buffer is written up to
    picture 1 only."""
    w, h, out = 320, 240, "YU64"
    samples = group_stream(source, w, h)
    want, _ = handle_pictures(samples, out, FULL)
    other = samples[6:8]                                         # (group 3 in place of group 0: pictures 0 and 1 change, nothing else may)
    q = GroupQueue(samples[0], out, FULL, 4)
    try:
        ret, status, first = q.decode(samples)
        assert ret == 8 and status == [0] * 8
        frame = q.row_bytes * q.h
        canary = np.full(frame * 8 + 64, 0x5a, np.uint8)
        blob, offsets, sizes = pack(other)
        assert q.submit(blob, offsets, sizes, canary, frame, q.row_bytes) == 0, amd_last_error()
        assert q.wait(2) == (2, [0, 0])
        for i in range(2): _same(canary[i * frame: (i + 1) * frame], want[6 + i][1], "short pass, picture %d" % i)
        assert (canary[2 * frame:] == 0x5a).all(), "the short pass wrote behind picture 1"
        after = q.pictures(8)
        for i in range(2): _same(after[i], want[6 + i][1], "short pass, download_output(%d)" % i)
        for i in range(2, 8): _same(after[i], first[i], "download_output(%d) behind the short pass" % i)
    finally:
        q.close()


# ---- 7. a verdict per pair
def damaged_group(kind, sample, other):
    """decode_queue.damaged for a group sample.  The kinds behind its count of an intra sample's 27 bands are restated, the two that name bands for a group: it has 51 band headers (17 per channel, the temporal wavelet's empty
    one included) where an intra sample has 27, and its longest payload is subband 7's raw words, which no pattern makes undecodable -- the pattern goes into the
    longest run-length coded band."""
    if kind in ("cut in half", "frame width"): return damaged(kind, sample, other)
    if kind == "other geometry": return other, len(other)
    if kind == "two bytes": return sample[:2], 2
    assert kind in ("size chunk", "payload pattern"), kind
    s = bytearray(sample)
    if kind == "size chunk":
        bands = walk_bands(sample)
        assert len(bands) == 51
        at = bands[-1][0]; s[at: at + 4] = b"\x20\xff\xff\xff"
    else:
        _, _, _, lo, hi = max((b for b in group_bands(sample) if b[2] == 3), key=lambda b: b[4] - b[3])
        at = (lo + (hi - lo) // 2) & ~3; s[at: at + 64] = bytes((i * 37 + 11) & 0xff for i in range(64))
    return bytes(s), len(s)


def damaged_follower(kind, sample):
    if kind == "first tag": return b"\x00\x03" + sample[2:], len(sample)
    if kind == "two bytes": return sample[:2], 2
    if kind == "size 0": return sample, 0
    raise ValueError(kind)


def check_verdicts(kind, follower_kind, source="ref"):
    """Group 1 of 4 damaged as `kind` says, follower 2 as `follower_kind` says: statuses and pictures are the handle's in order, the untouched pairs byte for byte what
    an intact pass gives."""
    w, h, out = 320, 240, "YU64"
    intact = list(group_stream(source, w, h))
    other = group_stream(source, 336, 252)[0]
    samples = list(intact); sizes = [len(s) for s in samples]
    samples[2], sizes[2] = damaged_group(kind, intact[2], other)
    samples[5], sizes[5] = damaged_follower(follower_kind, intact[5])
    want, _ = handle_pictures(samples, out, FULL, sizes=sizes, first=intact[0])
    codes = [rc for rc, _ in want]
    print("%s / %s: the handle answers %s" % (kind, follower_kind, codes))
    assert codes[2] != 0, "'%s' left the group decodable on the handle: choose another" % kind
    assert codes[5] != 0, "'%s' left the follower decodable on the handle: choose another" % follower_kind
    assert [codes[i] for i in (0, 1, 4, 6, 7)] == [0] * 5
    good, _ = handle_pictures(intact, out, FULL)
    q = GroupQueue(intact[0], out, FULL, 4)
    try:
        blob, offsets, _ = pack(samples)
        assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
        ret, status = q.wait(8)
        pictures = q.pictures(8)
        assert status == codes, (status, codes)
        assert ret == status.count(0)
        for i in range(8):
            _same(pictures[i], want[i][1], "%s / %s: sample %d" % (kind, follower_kind, i))
            if status[i]: assert not pictures[i].any(), "sample %d failed and its picture is not zero" % i
        for i in (0, 1, 6, 7): _same(pictures[i], good[i][1], "the untouched pair of sample %d" % i)
        # the same pass with its pictures to host memory
        frame = q.row_bytes * q.h; host = np.full(frame * 8, 9, np.uint8)
        assert q.submit(blob, offsets, sizes, host, frame, q.row_bytes) == 0, amd_last_error()
        assert q.wait(8) == (ret, status)
        for i, p in enumerate(q.pictures(8)):
            _same(host[i * frame: (i + 1) * frame], want[i][1], "host picture %d" % i)
            _same(p, want[i][1], "download_output(%d) behind a pass with host pictures" % i)
        # an intact pass on the same batch afterwards
        ret, status, pictures = q.decode(intact)
        assert ret == 8 and status == [0] * 8
        for i in range(8): _same(pictures[i], good[i][1], "intact pass behind the damaged one: sample %d" % i)
    finally:
        q.close()


def check_sequence_header_as_a_sample(source="amd"):
    """A sequence header passed in a group's place: the handle answers OKAY without a picture, the queue gives a zero picture (and the follower has no group)."""
    w, h, out = 320, 240, "YU64"
    intact = list(group_stream(source, w, h))
    frames = [np.ascontiguousarray(DQ._yuy2_frame(w, h, i, False)) for i in range(2)]
    header = (ref_encode_frames if source == "ref" else amd_encode_frames)(frames, w * 2, w, h, PIX_YUY2, ENCODED_YUV422, QUALITY_FILMSCAN1, GOP)[0]
    assert len(header) == 40
    samples = list(intact); samples[2] = header
    want, _ = handle_pictures(samples, out, FULL, first=intact[0])
    assert want[2][0] == 0 and want[3][0] != 0
    q = GroupQueue(intact[0], out, FULL, 4)
    try:
        ret, status, pictures = q.decode(samples)
        assert status == [rc for rc, _ in want] and ret == status.count(0), status
        assert not pictures[2].any() and not pictures[3].any()
        for i in (0, 1, 4, 5, 6, 7): _same(pictures[i], want[i][1], "sample %d" % i)
    finally:
        q.close()


# ---- 8. queue
def check_queue(source="ref"):
    w, h = 320, 240
    sets = [group_stream(source, w, h), group_stream(source, w, h, 1)]
    outs = ["YU64", "RG48"]
    want = [handle_pictures(s, o, FULL)[0] for s, o in zip(sets, outs)]
    L = lib()
    qs = [GroupQueue(s[0], o, FULL, 4) for s, o in zip(sets, outs)]
    try:
        packed = [pack(s) for s in sets]
        synchronous = []
        for q, s in zip(qs, sets): synchronous.append(q.decode(s)[2])
        for step in range(2):
            for q, (blob, offsets, sizes) in zip(qs, packed): assert q.submit(blob, offsets, sizes) == 0, amd_last_error()
            q = qs[0]; blob, offsets, sizes = packed[0]
            buf = np.zeros(q.row_bytes * q.h, np.uint8); x = ctypes.c_int()
            assert q.submit(blob, offsets, sizes) == -1
            assert L.cfhd_amd_decode_batch_submit_device(q.b, blob.ctypes.data_as(V), blob.nbytes, _sizes(offsets), _sizes(sizes), 8) == -1
            assert L.cfhd_amd_decode_batch_geometry(q.b, ctypes.byref(x), None, None) == -1
            assert L.cfhd_amd_decode_batch_download_output(q.b, 0, buf.ctypes.data_as(V), q.row_bytes) == -1
            assert L.cfhd_amd_decode_batch_kernel_ms(q.b, 0) == 0 and L.cfhd_amd_decode_batch_kernel_name(q.b, 0) == b""
            for k, q in enumerate(qs):
                assert q.wait(8) == (8, [0] * 8)
                for i, p in enumerate(q.pictures(8)):
                    _same(p, want[k][i][1], "batch %d step %d sample %d" % (k, step, i))
                    _same(p, synchronous[k][i], "batch %d step %d sample %d against the synchronous pass" % (k, step, i))
            assert L.cfhd_amd_decode_batch_wait(qs[0].b, None) == -1                  # nothing in flight
        names = [L.cfhd_amd_decode_batch_kernel_name(qs[0].b, k).decode() for k in range(8)]
        assert names[0] == "k_dec_ingest" and names[1] == "k_dec_parse_group" and "k_dec_band_two_pass" in names[2] and names[3] == "k_dec_lowpass" and names[7] == "k_dec_blank" and all(names), names
        ms = [L.cfhd_amd_decode_batch_kernel_ms(qs[0].b, k) for k in range(9)]
        assert all(x >= 0 for x in ms) and sum(ms) > 0 and L.cfhd_amd_decode_batch_kernel_ms(qs[0].b, 9) == 0, ms
        blob, offsets, sizes = packed[1]
        assert qs[1].submit(blob, offsets, sizes) == 0
        qs[1].close()                                            # destroy on a batch in flight returns
    finally:
        for q in qs: q.close()


# ---- 9. gates
def refused(sample, out, resolution, ngroups):
    L = lib()
    fb = ctypes.create_string_buffer(sample, len(sample))
    b = L.cfhd_amd_decode_batch_create_groups(fb, len(sample), FOURCCS[out], resolution, ngroups)
    if b: L.cfhd_amd_decode_batch_destroy(b); return False
    text = amd_last_error()
    assert text, "refused without a text"
    return text


def check_gates():
    w, h = 320, 240
    frames = [np.ascontiguousarray(DQ._yuy2_frame(w, h, i, False)) for i in range(3)]
    stream = amd_encode_frames(frames, w * 2, w, h, PIX_YUY2, flags=GOP)
    header, group, follower = stream
    assert len(header) == 40 and len(follower) == 24
    intra = amd_encode_frames(frames[:1], w * 2, w, h)[0]
    interlaced = group_stream("amd", w, h, 1)[0]
    assert "sequence header" in refused(header, "YUY2", FULL, 4)
    assert "P-frame" in refused(follower, "YUY2", FULL, 4)
    assert "intra" in refused(intra, "YUY2", FULL, 4)
    # the handle's refusal with the text create gives for an intra sample the handle refuses: an interlaced group to YU64 at full resolution (CFHD_ERROR_BADFORMAT)
    text = refused(interlaced, "YU64", FULL, 4)
    assert text == "decode queue: CFHD_DecodeSample refuses this sample, output and resolution (CFHD_Error 3)", text
    assert "CFHD_Error 11" in refused(group, "YUY2", QUARTER, 4), "quarter resolution"
    assert "ngroups" in refused(group, "YUY2", FULL, 0)
    assert "grid limit" in refused(group, "YUY2", FULL, 20000)
    # the intra entry point keeps refusing group streams
    assert "group" in DQ.refused(group, "YUY2", FULL, 4) and "group" in DQ.refused(header, "YUY2", FULL, 4)
    q = GroupQueue(group, "YUY2", FULL, 2)
    try:
        blob, offsets, sizes = pack([group, follower, group])
        assert q.submit(blob, offsets, sizes) == -1, "an odd count"
        L = lib()
        assert L.cfhd_amd_decode_batch_submit_device(q.b, blob.ctypes.data_as(V), blob.nbytes, _sizes(offsets), _sizes(sizes), 3) == -1
        blob, offsets, sizes = pack([group, follower] * 3)
        assert q.submit(blob, offsets, sizes) == -1, "more than 2 * ngroups samples"
        ret, status, _ = q.decode([group, follower])
        assert (ret, status) == (2, [0, 0])
    finally:
        q.close()


def gates_under_host_entropy():
    """Child process body (CFHD_AMD_ENTROPY=host is read when the library starts its first encoder): the queue refuses, the handle still decodes."""
    w, h = 320, 240
    frames = [np.ascontiguousarray(DQ._yuy2_frame(w, h, i, False)) for i in range(2)]
    group = amd_encode_frames(frames, w * 2, w, h, PIX_YUY2, flags=GOP)[1]
    text = refused(group, "YUY2", FULL, 4)
    assert text and "CFHD_AMD_ENTROPY" in text, text
    amd_decode_sample(group)
    print("HOST ENTROPY REFUSED")
