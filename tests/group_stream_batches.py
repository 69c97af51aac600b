"""One GROUP encoder's stream on the frame queue, rate feedback included -- cfhd_amd_batch_create_group_stream: the helpers and test bodies shared by
tests/test_gpu_group_stream_batches.py (hardware) and tests/test_group_stream_batches_emulated.py (the same functions inside cfhd_testlib.emulated_product()).
The group twin of tests/stream_batches.py; "frame" reads "group".

What is checked against what:
  samples   the sequence header + the batch's samples, pass behind pass (group, 24-byte P-frame sample, group, ...), against ONE CFHD_EncodeSample handle of this
            library with CFHD_AMD_ENTROPY=device (a group the handle would hand to the host writer fails the call instead) and against the reference encoder, both
            prepared with the group flag and fed the same frames: equal sizes, equal bytes after mask_volatile_metadata.
  stats     cfhd_amd_batch_stream_stats against the table changes counted in the reference's own stream (tests/hooks/group_stream_hooks.cpp reads a group
            sample's divisors).
  pictures  (mode 0) one CFHD_DecodeSample handle over the same samples (group_batches.cabi_group_pictures): 16-bit outputs word for word, 8-bit 4:2:2 within the
            one dither step.
The inputs are judged on the reference's samples alone, on the CPU, before the product is asked anything (check_input_does_its_job, limiter_input_does_its_job).
Test infrastructure only: nothing here is a product path."""
import ctypes, os, subprocess, sys
import numpy as np
from cfhd_testlib import *
import cfhd_testlib as T
import quality_matrix as Q
import group_batches as GB
import stream_batches as S

V = ctypes.c_void_p
FILMSCAN2, FILMSCAN3, MEDIUM, HIGH = 5, 6, 2, 3
INTERLACED, GOP = 1, ENCODING_FLAGS_2FRAME_GOP
W, H, N, PASSES = 192, 96, 8, 3
NG = N // 2
# route: (input, width, interlaced, mode, noise amplitude of the route's noisy groups) -- every family of the group encoder's loaders: 8-bit 4:2:2 (progressive, and the frame transform of interlaced groups with
# its difference-coded bands), v210 (whole 48-pixel groups: 384), 16-bit RGB through the colour conversion, 8-bit RGB with subband 7 coded in two passes, an Avid
# layout (no decoder output: mode 1)
ROUTES = {"YUY2": ("YUY2", W, 0, 0, 1), "YUY2-i": ("YUY2", W, 1, 0, 0), "v210": ("v210", 384, 0, 0, 1), "RG48": ("RG48", W, 0, 0, 1), "BGRA": ("BGRA", W, 0, 0, 1), "a214": ("a214", W, 0, 1, 1)}
STREAM_CASES = [(r, q) for r in ROUTES for q in (FILMSCAN2, FILMSCAN3)]
FOURCCS = dict(GB.FOURCCS)
# SCHEDULE[g % 12]: the kind of both frames of the group at stream index g -- 0: one grey level (noisy_frame with amplitude -1), the smallest group sample there is;
# 1: gradients plus uniform noise of the route's amplitude (in 8-bit steps; 0: the gradients alone, which the field shear of the interlaced route makes large enough).
# What the search against the reference encoder alone showed (tried_schedules() prints the walk: sizes and a letter per table set), all at 192 x 96:
#   * The FILMSCAN2 / 3 limiter (cfhd_tables.cpp derive_subband_tables) moves on every CALL, so every key sample's size is applied twice -- on the call that opens the
#     next group, whose tables it moves, and on the call that completes it, which shows in the group after.  It spans 0 .. 20, the tables follow it up to 16.
#   * It reads the group sample as ONE frame's bytes: 192 x 96 x 2.5 / size.  A group sample of a 10-bit source is never smaller than 10 808 bytes here (grey frames:
#     headers and the raw 16-bit lowpass bands of w[5] and w[3]; 16 916 at 384 x 96), compression 4.26 -- inside the dead band of both words (4 .. 5.5 | 3 .. 4.5).  The
#     only smaller key sample is the 40-byte sequence header, which takes the limiter down by 4 behind group 0: the one step to finer tables such a stream has.  (BGRA
#     codes subband 7 and gets down to 6 696 bytes, v210 at FILMSCAN3 sits just past 4.5: those go down behind every grey group.)
#   * The stream_batches schedule (gradients 0, noise 6 / 16) saturates the limiter within two groups on every route: the gradients alone are 11 900 bytes, compression
#     3.87, one step up a call at FILMSCAN2; noise 6 is 45 000 bytes, seven steps a call.  Noise 12 / 16 also puts v210 past the 80 % mark (142 624 / 148 960 bytes).
#   * Noise 1 behind grey groups (24 000 .. 36 000 bytes, two to four steps a call) holds on every route at both words except interlaced YUY2 at FILMSCAN2, where it
#     saturates at once (33 200 bytes, compression 1.39); the gradients alone (16 600 bytes) do there.  Noise 2 and 3 stand still across the boundary in front of group 8.
# The noisy groups sit in front of the pass boundaries (groups 3 and 7) and inside the last pass (group 10).
SCHEDULE = (0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0)


def lib():
    L = S.lib()
    if not getattr(L, "_group_stream_batches_declared", False):
        L.cfhd_amd_batch_create_group_stream.restype = V
        L.cfhd_amd_batch_create_group_stream.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_int] * 4
        L.cfhd_amd_batch_create_groups.restype = V
        L.cfhd_amd_batch_create_groups.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_int] * 4
        L.cfhd_amd_batch_get_sequence_header.argtypes = [V, ctypes.POINTER(V), ctypes.POINTER(ctypes.c_size_t)]
        L._group_stream_batches_declared = True
    return L


GROUP_HOOKS_SO = os.path.join(T.ROOT, "tests", "_build", "libcfhd_group_stream_hooks.so")
_group_hooks = None


def group_hooks():
    """Test-only library: tests/hooks/group_stream_hooks.cpp + the product's host-only sources, built the way cfhd_testlib.hooks() builds its library."""
    global _group_hooks
    if _group_hooks is None:
        csrc = os.path.join(T.PRODUCT_DIR, "csrc")
        srcs = [os.path.join(T.ROOT, "tests", "hooks", "group_stream_hooks.cpp")] + [os.path.join(csrc, f) for f in ("cfhd_tables.cpp", "cfhd_bitstream.cpp", "cfhd_metadata.cpp", "cfhd_gop.cpp")]
        deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        if not os.path.exists(GROUP_HOOKS_SO) or any(os.path.getmtime(d) > os.path.getmtime(GROUP_HOOKS_SO) for d in deps):
            os.makedirs(os.path.dirname(GROUP_HOOKS_SO), exist_ok=True)
            T._build_once(GROUP_HOOKS_SO, ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, "-I" + os.path.join(T.ROOT, "include")] + srcs, deps)
        L = ctypes.CDLL(GROUP_HOOKS_SO)
        L.cfhd_amd_group_sample_quants.argtypes = [c_u8p, ctypes.c_size_t, c_intp]
        _group_hooks = L
    return _group_hooks


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def pitch_of(fmt, w): return {"YUY2": 2 * w, "2vuy": 2 * w, "v210": (w + 47) // 48 * 128, "RG48": 6 * w, "BGRA": 4 * w, "a214": 4 * w}[fmt]


def noisy_frame(fmt, w, h, index, amplitude, interlaced=False):
    """stream_batches.noisy_frame's picture -- gradients that move a little with the index plus uniform noise of the given amplitude (8-bit steps) -- in the inputs of
    the group encoder; amplitude < 0: no gradients either, one grey level that moves with the index (the smallest group samples there are)."""
    rng = np.random.default_rng(900 + index)
    y, x = np.mgrid[0:h, 0:w]
    comps = []
    for k in range(3):
        g = 128.0 + (36.0 - 6.0 * k) * np.sin((x + 3.0 * index) / (61.0 + 17.0 * k)) * np.cos((y + 5.0 * k) / (47.0 + 11.0 * k))
        if amplitude < 0: g = np.full((h, w), 120.0 + index % 7)
        if interlaced: g[1::2] = np.roll(g[1::2], 2, axis=1)
        comps.append(np.clip(g + (rng.integers(-amplitude, amplitude + 1, (h, w)) if amplitude > 0 else 0), 1, 254))
    if fmt == "YUY2":
        f = np.zeros((h, w * 2), np.uint8)
        f[:, 0::2] = comps[0]; f[:, 1::4] = comps[1][:, 0::2]; f[:, 3::4] = comps[2][:, 0::2]
    elif fmt == "RG48":
        f = np.stack([(c * 256.0).astype(np.uint16) for c in comps], axis=2).reshape(h, -1).view(np.uint8)
    elif fmt == "2vuy":
        f = np.zeros((h, w * 2), np.uint8)
        f[:, 1::2] = comps[0]; f[:, 0::4] = comps[1][:, 0::2]; f[:, 2::4] = comps[2][:, 0::2]
    elif fmt == "BGRA":
        f = np.full((h, w, 4), 255, np.uint8)
        for k in range(3): f[:, :, 2 - k] = comps[k]
        f = f.reshape(h, -1)
    elif fmt == "v210":                                  # six pixels in four little-endian words of three 10-bit fields: Cb Y Cr | Y Cb Y | Cr Y Cb | Y Cr Y
        assert w % 48 == 0
        Y = (comps[0] * 4).astype(np.uint32); Cb = (comps[1][:, 0::2] * 4).astype(np.uint32); Cr = (comps[2][:, 0::2] * 4).astype(np.uint32)
        f = np.zeros((h, w // 6 * 4), np.uint32)
        f[:, 0::4] = Cb[:, 0::3] | (Y[:, 0::6] << 10) | (Cr[:, 0::3] << 20)
        f[:, 1::4] = Y[:, 1::6] | (Cb[:, 1::3] << 10) | (Y[:, 2::6] << 20)
        f[:, 2::4] = Cr[:, 1::3] | (Y[:, 3::6] << 10) | (Cb[:, 2::3] << 20)
        f[:, 3::4] = Y[:, 4::6] | (Cr[:, 2::3] << 10) | (Y[:, 5::6] << 20)
        f = f.view(np.uint8)
    elif fmt == "a214":                                  # int16 words Cb Y Cr Y, the inverse of the reference's scaling (avid_frames.frame)
        y10 = (comps[0] * 4).astype(np.int64); cb = (comps[1][:, 0::2] * 4).astype(np.int64); cr = (comps[2][:, 0::2] * 4).astype(np.int64)
        f = np.zeros((h, 2 * w), np.int64)
        f[:, 1::2] = (y10 - 64) * 16384 // (219 * 4)
        f[:, 0::4] = (cb - 64) * 16384 // (224 * 4) - 8192; f[:, 2::4] = (cr - 64) * 16384 // (224 * 4) - 8192
        f = np.clip(f, -32768, 32767).astype(np.int16).view(np.uint8)
    else: raise KeyError(fmt)
    f = np.ascontiguousarray(f).reshape(-1)
    assert f.size == pitch_of(fmt, w) * h, (fmt, f.size)
    f.setflags(write=False)
    return f


def stream_frames(fmt, w, h, interlaced, nframes, passes, noise, schedule=None):
    schedule = SCHEDULE if schedule is None else schedule
    return [noisy_frame(fmt, w, h, i, noise if schedule[(i // 2) % len(schedule)] else -1, bool(interlaced)) for i in range(nframes * passes)]


def ref_group_stream(frames, pitch, w, h, fmt, interlaced, quality):
    """The reference's stream of one handle prepared with the group flag: [sequence header, group 0, P-frame sample, group 1, ...] -- one call more than there are
    frames, which brings the last P-frame sample out."""
    return ref_encode_frames(list(frames) + [frames[0]], pitch, w, h, pixfmt=FOURCCS[fmt], quality=quality, flags=GOP | (INTERLACED if interlaced else 0))


def handle_group_stream(frames, pitch, w, h, fmt, interlaced, quality):
    """The same through one CFHD_EncodeSample handle of this library, CFHD_AMD_ENTROPY=device."""
    with GB.device_entropy():
        return amd_encode_frames(list(frames) + [frames[0]], pitch, w, h, FOURCCS[fmt], quality=quality, flags=GOP | (INTERLACED if interlaced else 0))


_streams = {}


def stream(route, quality):
    """(frames of PASSES passes, pitch, the reference's stream through one handle) -- computed once, shared, read-only."""
    key = (route, quality)
    if key not in _streams:
        fmt, w, interlaced, _, noise = ROUTES[route]
        frames = stream_frames(fmt, w, H, interlaced, N, PASSES, noise)
        pitch = pitch_of(fmt, w)
        refs = ref_group_stream(frames, pitch, w, H, fmt, interlaced, quality)
        check_input_does_its_job(refs, NG, w, H, fmt, interlaced, "%s 0x%x" % (route, quality))
        _streams[key] = (frames, pitch, refs)
    return _streams[key]


def sample_tables(sample):
    out = (ctypes.c_int * 64)()
    a = np.frombuffer(sample, np.uint8).copy()
    n = group_hooks().cfhd_amd_group_sample_quants(p8(a), len(sample), out)
    assert n > 0, "cfhd_amd_group_sample_quants -> %d" % n
    return tuple(out[:n])


def groups_of(stream_samples):
    """The group samples of [sequence header, group, P-frame sample, ...]."""
    assert len(stream_samples[0]) == 40 and all(len(s) == 24 for s in stream_samples[2::2])
    return stream_samples[1::2]


def table_changes(stream_samples):
    """[g for which group g carries other tables than group g - 1], over a whole stream."""
    t = [sample_tables(s) for s in groups_of(stream_samples)]
    return [g for g in range(1, len(t)) if t[g] != t[g - 1]]


def sample_buffer_bytes(fmt, w, h):
    """cfhd_gop.cpp build_gop_plan: SampleEncoder.cpp:387 with the reference's own pixel sizes."""
    return w * h * {"YUY2": 4, "2vuy": 4, "BGRA": 4, "v210": 3, "RG48": 6}.get(fmt, 8) + 65536


def check_input_does_its_job(refs, ngroups, w, h, fmt, interlaced, what):
    """On the REFERENCE's stream alone: at least three distinct table sets, a change in each direction, a change across every pass boundary; no group sample at the
    reference's 80 % mark (gop_sample_may_zero_bands: the device stage does not write such a sample); interlaced groups: no band with more peaks than the device's
    positions hold -- two million, which a band of these geometries (at most 96 x 48 coefficients) cannot reach."""
    groups = groups_of(refs)
    t = [sample_tables(s) for s in groups]
    assert len(set(t)) >= 3, "%s: %d distinct table sets in the stream" % (what, len(set(t)))
    ups = [g for g in range(1, len(t)) if sum(t[g]) > sum(t[g - 1])]; downs = [g for g in range(1, len(t)) if sum(t[g]) < sum(t[g - 1])]
    assert ups and downs, "%s: tables coarser behind %s, finer behind %s" % (what, ups, downs)
    for k in range(ngroups, len(t), ngroups): assert t[k] != t[k - 1], "%s: the tables stand still across the boundary in front of group %d" % (what, k)
    for g, s in enumerate(groups): assert len(s) * 100 <= sample_buffer_bytes(fmt, w, h) * 80, "%s: group %d has %d bytes" % (what, g, len(s))
    if interlaced: assert (w // 2) * (h // 2) < (1 << 21)


def tried_schedules(schedule=None, noise=None, routes=None, qualities=(FILMSCAN2, FILMSCAN3)):
    """The search behind SCHEDULE, for reading: per route and word the sizes of the reference's group samples and a letter per distinct table set."""
    for route in (routes or ROUTES):
        fmt, w, interlaced, _, route_noise = ROUTES[route]
        frames = stream_frames(fmt, w, H, interlaced, N, PASSES, route_noise if noise is None else noise, schedule)
        for q in qualities:
            refs = ref_group_stream(frames, pitch_of(fmt, w), w, H, fmt, interlaced, q)
            t = [sample_tables(s) for s in groups_of(refs)]
            names = {}
            for x in t: names.setdefault(x, chr(ord("a") + len(names)))
            try: check_input_does_its_job(refs, NG, w, H, fmt, interlaced, route); ok = "ok"
            except AssertionError as e: ok = str(e)
            print("%-7s 0x%x  %s  %s  %s" % (route, q, "".join(names[x] for x in t), [len(s) for s in groups_of(refs)], ok))


# ------------------------------------------------------------------------------------------
# the batch
# ------------------------------------------------------------------------------------------
class Batch(GB.Batch):
    """One group-stream batch (or, entry="groups", one batch of cfhd_amd_batch_create_groups with the same arguments) with nframes slots; feed() puts a pass's frames
    into HBM."""
    def __init__(self, w, h, fmt, interlaced, quality, nframes, mode, entry="group_stream"):
        self.L = lib(); self.w, self.h, self.name, self.n, self.mode = w, h, fmt, nframes, mode
        create = self.L.cfhd_amd_batch_create_group_stream if entry == "group_stream" else self.L.cfhd_amd_batch_create_groups
        self.b = create(w, h, FOURCCS[fmt], INTERLACED if interlaced else 0, quality, nframes, 1, mode)
        assert self.b, "cfhd_amd_batch_create_%s -> NULL (%s)" % (entry, amd_last_error())
        self.pitch = pitch_of(fmt, w)

    def feed(self, frames):
        assert len(frames) == self.n
        for i, f in enumerate(frames):
            assert self.L.cfhd_amd_batch_upload(self.b, i, np.asarray(f).ctypes.data_as(V), self.pitch) == 0, amd_last_error()

    def stats(self):
        out = (ctypes.c_int * 3)(-7, -7, -7)
        rc = self.L.cfhd_amd_batch_stream_stats(self.b, out)
        return rc, list(out)

    def header(self):
        rc, h = GB.sequence_header(self.L, self.b)
        assert rc == 0 and len(h) == 40
        return h

    def pictures(self):
        out = []
        for i in range(self.n):
            o = np.full(self.pitch * self.h, 7, np.uint8)
            assert self.L.cfhd_amd_batch_download_output(self.b, i, o.ctypes.data_as(V), self.pitch) == 0, amd_last_error()
            out.append(o)
        return out


def run_stream(bt, frames, passes, queued=False):
    """[(samples, stats, pictures or None)] of `passes` passes over consecutive runs of bt.n frames."""
    out = []
    for k in range(passes):
        bt.feed(frames[k * bt.n: (k + 1) * bt.n])
        if queued:
            assert bt.L.cfhd_amd_batch_submit(bt.b) == 0, amd_last_error()
            total = bt.L.cfhd_amd_batch_wait(bt.b)
        else: total = bt.L.cfhd_amd_batch_roundtrip(bt.b)
        assert total > 0, "pass %d -> %d (%s)" % (k, total, amd_last_error())
        s = bt.samples()
        assert total == sum(len(x) for x in s[0::2]) and all(len(x) == 24 for x in s[1::2])
        rc, st = bt.stats()
        assert rc == 0, "cfhd_amd_batch_stream_stats -> %d" % rc
        out.append((s, st, bt.pictures() if bt.mode == 0 else None))
    return out


def check_pictures(samples, pictures, fmt, what):
    """The batch's pictures against one CFHD_DecodeSample handle over the same samples: 16-bit outputs word for word, the dithered 8-bit outputs (4:2:2, and BGRA as
    tests/group_batches_rgb8.py judges it) within the one dither step."""
    if fmt == "BGRA": want, aw, ah, pitch = GB.cabi_group_pictures(samples, fmt)      # (the handle decodes the two passes of subband 7 on the host: tests/group_batches_rgb8.py)
    else:
        with GB.device_entropy(): want, aw, ah, pitch = GB.cabi_group_pictures(samples, fmt)
    for i, pic in enumerate(want):
        assert pic.size == pictures[i].size, (what, i, aw, ah, pitch)
        if fmt in ("YUY2", "2vuy", "BGRA"):              # the dithered 8-bit outputs
            d = np.abs(pictures[i].astype(np.int16) - pic.astype(np.int16))
            assert d.max() <= 1, "%s picture %d: %d bytes further than one dither step from the handle's" % (what, i, int((d > 1).sum()))
        else:
            a, b = pictures[i].view(np.uint16), pic.view(np.uint16)
            assert np.array_equal(a, b), "%s picture %d: %d words differ from the handle's picture" % (what, i, int((a != b).sum()))


def check_stats(stats, refs, nframes, what):
    """Σ out[2] is the number of table changes in the reference's stream; a window that starts behind group 0 ran; the bounds of out[1]."""
    assert sum(st[2] for st in stats) == len(table_changes(refs)), what + "stats %s, table changes in the reference's stream in front of groups %s" % (stats, table_changes(refs))
    assert any(st[0] >= 2 and st[1] < nframes * st[0] for st in stats), what + "no pass re-coded a window that starts behind group 0: %s" % stats
    for st in stats: assert nframes <= st[1] <= nframes * st[0] and st[1] % 2 == 0, what + "stats %s" % stats


# ------------------------------------------------------------------------------------------
# 1. FILMSCAN2 / FILMSCAN3 streams; 2. one more geometry
# ------------------------------------------------------------------------------------------
def compare_stream(bt, frames, passes, refs, handle, fmt, what, nframes):
    header = bt.header()
    res = run_stream(bt, frames, passes, queued=True)
    mine = [header] + [s for p in res for s in p[0]]
    assert len(mine) == len(refs) == len(handle)
    Q.assert_samples_equal(mine, handle, what + "against this library's handle: ")
    Q.assert_samples_equal(mine, refs, what + "against the reference: ")
    check_stats([p[1] for p in res], refs, nframes, what)
    if bt.mode == 0:
        for k, p in enumerate(res): check_pictures(p[0], p[2], fmt, what + "pass %d" % k)
    return res


def check_stream(route, quality):
    fmt, w, interlaced, mode, _ = ROUTES[route]
    what = "%s 0x%x: " % (route, quality)
    frames, pitch, refs = stream(route, quality)
    L = lib()
    assert L.cfhd_amd_quantizer_is_static(w, H, FOURCCS[fmt], 0, GOP | (INTERLACED if interlaced else 0), quality) == 0
    handle = handle_group_stream(frames, pitch, w, H, fmt, interlaced, quality)
    bt = Batch(w, H, fmt, interlaced, quality, N, mode)
    try:
        assert bt.stats()[0] == -1                      # (no pass has completed)
        compare_stream(bt, frames, PASSES, refs, handle, fmt, what, N)
    finally:
        bt.close()


# 336 x 252 2vuy: odd chroma lowpass widths (336 / 2 / 8 = 21) and a display height that is no multiple of 8; six frames a pass
GEOMETRY = (336, 252, "2vuy", 6)
GEOMETRY_SCHEDULE, GEOMETRY_NOISE = (0, 0, 1, 0, 0, 1, 0, 1, 0), 1      # (three groups a pass: the noisy groups in front of the boundaries, groups 2 and 5, and group 7)
_geometry = []


def check_other_geometry():
    w, h, fmt, n = GEOMETRY
    if not _geometry:
        frames = stream_frames(fmt, w, h, 0, n, PASSES, GEOMETRY_NOISE, GEOMETRY_SCHEDULE)
        refs = ref_group_stream(frames, 2 * w, w, h, fmt, 0, FILMSCAN2)
        check_input_does_its_job(refs, n // 2, w, h, fmt, 0, "%d x %d %s" % (w, h, fmt))
        _geometry.append((frames, refs))
    frames, refs = _geometry[0]
    handle = handle_group_stream(frames, 2 * w, w, h, fmt, 0, FILMSCAN2)
    bt = Batch(w, h, fmt, 0, FILMSCAN2, n, 0)
    try:
        compare_stream(bt, frames, PASSES, refs, handle, fmt, "%d x %d %s: " % (w, h, fmt), n)
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------
# 3. a settled stream; 4. a static word through the new entry (the traces: tests/test_group_stream_batches_emulated.py)
# ------------------------------------------------------------------------------------------
def settle(bt, frame, limit=8):
    """Passes over copies of one frame until the tables stop moving -- the FILMSCAN2 / 3 limiter moves at least a step a call while the key sample's size lies outside
    its band and spans 0 .. 20 --; returns the stats of every pass."""
    stats = []
    for k in range(limit):
        bt.feed([frame] * bt.n)
        assert bt.L.cfhd_amd_batch_roundtrip(bt.b) > 0, amd_last_error()
        rc, st = bt.stats()
        assert rc == 0
        stats.append(st)
        if st[2] == 0 and k: return stats
    raise AssertionError("the tables still move after %d passes over one frame: %s" % (limit, stats))


def check_still_pass(fmt="YUY2"):
    frame = noisy_frame(fmt, W, H, 0, 6)
    bt = Batch(W, H, fmt, 0, FILMSCAN2, N, 1)
    try:
        header = bt.header()
        stats = settle(bt, frame)
        for k in range(2):
            bt.feed([frame] * N)
            assert bt.L.cfhd_amd_batch_roundtrip(bt.b) > 0, amd_last_error()
            assert bt.stats() == (0, [1, N, 0]), (stats, bt.stats())
        tail = bt.samples()
    finally:
        bt.close()
    # (and the settled stream is still the handle's: its last pass against the end of one handle's stream of as many copies)
    handle = handle_group_stream([frame] * (N * (len(stats) + 2)), pitch_of(fmt, W), W, H, fmt, 0, FILMSCAN2)
    assert header == handle[0]
    Q.assert_samples_equal(tail, handle[-N:], "the settled pass against the handle: ")


STATIC_CASES = ["YUY2", "BGRA"]


def check_static_word(route):
    """FILMSCAN1 through the new entry: cfhd_amd_batch_create_groups' samples and pictures (GUID pinned, DATE / TIME masked), stats [1, n, 0]."""
    fmt, w, interlaced, mode, _ = ROUTES[route]
    L = lib()
    assert L.cfhd_amd_quantizer_is_static(w, H, FOURCCS[fmt], 0, GOP, QUALITY_FILMSCAN1) == 1
    L.cfhd_amd_set_clip_guid(bytes(range(16)))
    frames = [noisy_frame(fmt, w, H, i, 6) for i in range(2 * N)]
    mine = Batch(w, H, fmt, interlaced, QUALITY_FILMSCAN1, N, 0); theirs = Batch(w, H, fmt, interlaced, QUALITY_FILMSCAN1, N, 0, entry="groups")
    try:
        assert theirs.stats()[0] == -1 and mine.header() == theirs.header()
        for k in range(2):
            for bt in (mine, theirs): bt.feed(frames[k * N: (k + 1) * N])
            assert mine.roundtrip() == theirs.roundtrip()
            Q.assert_samples_equal(mine.samples(), theirs.samples(), "%s pass %d, create_group_stream against create_groups: " % (route, k))
            assert all(np.array_equal(a, b) for a, b in zip(mine.pictures(), theirs.pictures()))
            assert mine.stats() == (0, [1, N, 0]) and theirs.stats()[0] == -1
    finally:
        mine.close(); theirs.close()


# ------------------------------------------------------------------------------------------
# 5. the bit-rate limiter (GPU only)
# ------------------------------------------------------------------------------------------
LIMITER_N, LIMITER_PASSES = 6, 2
LIMITER_BOUND = S.LIMITER_BOUND                          # bits a second at the limiter's 30 fps (cfhd_tables.cpp limit_bitrate)
# The limiter of a group encoder reads the size of the key sample in front as TWO frames' bits (cfhd_tables.cpp bitrate_of_previous_sample(st, framerate, 2)), so a
# group sample passes 1.2 x the bound from 1 500 000 (HIGH) | 1 300 000 (MEDIUM) bytes on.  LIMITER_GEOMETRY: the smallest geometry found, with the reference encoder
# on the CPU (limiter_search() is the search), at which limiter_input_does_its_job holds at BOTH words.  Tried, by area, on frames of about 16:9 with widths that are
# multiples of 16 (bytes of the two noisy group samples, HIGH | MEDIUM):
#   1152 x 648   1 553 924, 1 407 052 (too small) | 1 212 876 (too small), ..   1216 x 688   1 741 720, 1 576 536 | 1 359 644, 1 218 536 (too small)
#   1232 x 696   1 788 816, 1 620 136 | 1 397 328, 1 252 620 (too small)        1248 x 704   1 830 404, 1 656 852 | 1 428 676, 1 280 936 (too small)
#   1264 x 712   1 876 232, 1 698 900 | 1 464 796, 1 313 380                    1280 x 720   1 918 276, 1 736 432 | 1 497 064, 1 341 572
# At 1264 x 712 the six groups carry the table sets a b c b d a at both words: group 1 behind the first noisy sample, group 2 behind the second, groups 3 and 4 -- flat
# behind flat -- still coarser, group 5 on the normal tables again.  (With a flat group in front and three noisy ones, as for intra frames, the stream does not come
# back within six groups: a a b c d c at 1280 x 720 and 1360 x 768.)  The largest sample is 44 % of the sample buffer.
LIMITER_GEOMETRY = (1264, 712)


def limiter_frames(w, h):
    """Two noisy groups (four of feedback_test_frames), four flat ones: 12 frames.  The limiter runs on the call that opens a group and counts up once for a key sample
    past the bound and once more past 1.2 x the bound, down by one for each one below: two noisy groups leave it at 3, and groups 3 and 4 -- flat behind flat -- still
    carry coarser tables before group 5 is back on the normal ones.  (A flat group in front, as for intra frames, leaves no room for that in six groups.)"""
    flat = np.full(w * h * 2, 128, np.uint8)
    return feedback_test_frames(w, h, 4) + [flat] * 8


_limiter = {}


def limiter_stream(quality, w, h):
    key = (quality, w, h)
    if key not in _limiter:
        frames = limiter_frames(w, h)
        refs = ref_group_stream(frames, w * 2, w, h, "YUY2", 0, quality)
        limiter_input_does_its_job(refs, quality, w, h)
        _limiter[key] = (frames, refs)
    return _limiter[key]


def limiter_input_does_its_job(refs, quality, w, h):
    """On the reference's stream: the noisy group samples beyond 1.2 x the bound (two frames' worth), a flat group behind a flat group still on the coarser tables (the
    hysteresis of overbitrate, not only the tables of the group behind a large sample), the last group on the normal tables again; no group at the 80 % mark."""
    groups = groups_of(refs)
    t = [sample_tables(s) for s in groups]
    normal = t[0]
    for g in (0, 1): assert len(groups[g]) * 8 * 30 > 2 * 1.2 * LIMITER_BOUND[quality], "noisy group %d: %d bytes" % (g, len(groups[g]))
    assert t[1] != normal and t[2] != normal, "the limiter does not trip behind the noisy groups"
    # group 2 follows a large sample; groups 3, 4, .. follow flat (small) ones
    coarse = [g for g in range(3, len(t)) if t[g] != normal]
    assert len(coarse) >= 2, "flat groups behind flat groups that still carry the coarser tables: %s" % coarse
    assert t[-1] == normal, "the stream does not come back to the normal tables"
    for g, s in enumerate(groups): assert len(s) * 100 <= sample_buffer_bytes("YUY2", w, h) * 80, "group %d has %d bytes" % (g, len(s))


def limiter_search(geometries=((1152, 648), (1216, 688), (1232, 696), (1248, 704), (1264, 712), (1280, 720))):
    """For reading: per geometry and word the group sizes of the reference's stream, a letter per table set, and whether limiter_input_does_its_job holds."""
    for w, h in geometries:
        for q in (HIGH, MEDIUM):
            refs = ref_group_stream(limiter_frames(w, h), w * 2, w, h, "YUY2", 0, q)
            t = [sample_tables(s) for s in groups_of(refs)]
            names = {}
            for x in t: names.setdefault(x, chr(ord("a") + len(names)))
            try: limiter_input_does_its_job(refs, q, w, h); ok = "ok"
            except AssertionError as e: ok = str(e)
            print("%d x %d  quality %d  %s  %s  %s" % (w, h, q, "".join(names[x] for x in t), [len(s) for s in groups_of(refs)], ok))


def check_limiter(quality):
    """MEDIUM / HIGH on YUY2 groups at LIMITER_GEOMETRY: six frames a pass, two passes; the limiter trips inside pass 0 and lets go in pass 1."""
    w, h = LIMITER_GEOMETRY
    frames, refs = limiter_stream(quality, w, h)
    handle = handle_group_stream(frames, w * 2, w, h, "YUY2", 0, quality)
    bt = Batch(w, h, "YUY2", 0, quality, LIMITER_N, 1)
    try:
        header = bt.header()
        passes = run_stream(bt, frames, LIMITER_PASSES, queued=True)
    finally:
        bt.close()
    mine = [header] + [s for p in passes for s in p[0]]
    Q.assert_samples_equal(mine, handle, "quality %d against this library's handle: " % quality)
    Q.assert_samples_equal(mine, refs, "quality %d against the reference: " % quality)
    assert any(p[1][0] >= 2 for p in passes), [p[1] for p in passes]


# ------------------------------------------------------------------------------------------
# 6. queue; 7. gates
# ------------------------------------------------------------------------------------------
def check_queue():
    """Two group streams in flight -- one fed through submit_host from a registered buffer --, waited for in order: each is its own handle's stream.  Between submit and
    wait the shared entry points answer with their error values."""
    L = lib()
    cases = [("YUY2", FILMSCAN2), ("YUY2-i", FILMSCAN3)]
    streams = [stream(r, q) for r, q in cases]
    handles = [handle_group_stream(frames, pitch, W, H, "YUY2", ROUTES[r][2], q) for (frames, pitch, _), (r, q) in zip(streams, cases)]
    pitch = W * 2
    host = np.zeros(N * pitch * H, np.uint8)
    assert L.cfhd_amd_register_host_buffer(host.ctypes.data_as(V), host.nbytes) == 0
    bts = [Batch(W, H, "YUY2", ROUTES[r][2], q, N, 1) for r, q in cases]
    try:
        for j, bt in enumerate(bts): assert bt.header() == handles[j][0]
        for k in range(PASSES):
            bts[0].feed(streams[0][0][k * N: (k + 1) * N])
            host[:] = np.concatenate(streams[1][0][k * N: (k + 1) * N])
            assert L.cfhd_amd_batch_submit(bts[0].b) == 0, amd_last_error()
            assert L.cfhd_amd_batch_submit_host(bts[1].b, host.ctypes.data_as(V), pitch * H, pitch, None, 0, 0) == 0, amd_last_error()
            for bt in bts:
                p = V(); sz = ctypes.c_size_t(); buf = np.zeros(pitch * H, np.uint8); dx = (ctypes.c_uint32 * 16)()
                assert L.cfhd_amd_batch_roundtrip(bt.b) == -1 and L.cfhd_amd_batch_submit(bt.b) == -1
                assert L.cfhd_amd_batch_submit_host(bt.b, buf.ctypes.data_as(V), 0, pitch, None, 0, 0) == -1
                assert L.cfhd_amd_batch_upload(bt.b, 0, buf.ctypes.data_as(V), pitch) == -1
                assert L.cfhd_amd_batch_get_sample(bt.b, 0, ctypes.byref(p), ctypes.byref(sz)) == -1
                assert GB.sequence_header(L, bt.b)[0] == -1
                assert L.cfhd_amd_batch_download_output(bt.b, 0, buf.ctypes.data_as(V), pitch) == -1
                assert L.cfhd_amd_batch_kernel_ms(bt.b, 0) == 0 and L.cfhd_amd_batch_kernel_name(bt.b, 0) == b"" and L.cfhd_amd_batch_dx_stats(bt.b, dx) == -1
                assert bt.stats()[0] == -1
            for j, bt in enumerate(bts):
                total = L.cfhd_amd_batch_wait(bt.b)
                s = bt.samples()
                assert total == sum(len(x) for x in s[0::2]), (total, amd_last_error())
                Q.assert_samples_equal(s, handles[j][1 + k * N: 1 + (k + 1) * N], "batch %d pass %d: " % (j, k))
                assert bt.stats()[0] == 0
            assert L.cfhd_amd_batch_wait(bts[0].b) == -1          # nothing in flight
        assert L.cfhd_amd_batch_kernel_name(bts[0].b, 0) != b"" and L.cfhd_amd_batch_kernel_ms(bts[0].b, 6) >= 0
    finally:
        for bt in bts: bt.close()
        L.cfhd_amd_unregister_host_buffer(host.ctypes.data_as(V))


def refused(*a):
    """The text of a refusal, False for a batch that was made."""
    L = lib()
    b = L.cfhd_amd_batch_create_group_stream(*a)
    if b: L.cfhd_amd_batch_destroy(b); return False
    text = amd_last_error()
    assert text, "refused without a text"
    return text


def check_gates():
    L = lib()
    yuy2 = FOURCCS["YUY2"]
    for n in (7, 1, 0, -2): assert refused(W, H, yuy2, 0, FILMSCAN2, n, 1, 1), n
    assert refused(W, H, yuy2, 0, FILMSCAN2, N, 1, 2), "mode 2"
    assert refused(200, H, yuy2, 0, FILMSCAN2, N, 1, 1), "width 200"
    assert refused(W, H, yuy2, 0, 0, N, 1, 1), "a quality word with a low byte of 0"
    assert refused(384, H, FOURCCS["v210"], INTERLACED, FILMSCAN2, N, 1, 1), "interlaced groups: YUY2 / 2vuy"
    for name in ("RG64", "a214"): assert refused(W, H, FOURCCS[name], 0, FILMSCAN2, N, 1, 0), name + " has no decoder output"
    assert refused(W, H, fourcc("BYR4"), 0, FILMSCAN2, N, 1, 1), "Bayer frames do not encode to 4:2:2"
    for quality in (FILMSCAN2, FILMSCAN3, MEDIUM, HIGH, 1, QUALITY_FILMSCAN1):
        for mode in (0, 1): assert not refused(W, H, yuy2, 0, quality, N, 1, mode), (quality, mode)
    assert not refused(W, H, FOURCCS["BGRA"], 0, FILMSCAN2, 2, 1, 0) and not refused(W, H, yuy2, GOP | INTERLACED, FILMSCAN3, N, 1, 1)
    # cfhd_amd_batch_create_ex and cfhd_amd_batch_create_groups keep refusing the words whose group tables move: callers probe with them
    for quality in (FILMSCAN2, FILMSCAN3):
        for b in (L.cfhd_amd_batch_create_ex(W, H, yuy2, ENCODED_YUV422, GOP, quality, N, 1, 1), L.cfhd_amd_batch_create_groups(W, H, yuy2, 0, quality, N, 1, 1)):
            if b: L.cfhd_amd_batch_destroy(b)
            assert not b, quality
    # cfhd_amd_batch_create_stream keeps refusing the group flag, and keeps naming cfhd_amd_batch_create_groups
    assert "cfhd_amd_batch_create_groups" in S.refused(W, H, yuy2, ENCODED_YUV422, GOP, FILMSCAN2, N, 1, 1)
    # CFHD_AMD_HANDOFF=host (read when a batch is made): refused for moving words, taken for a word whose tables stand still
    old = os.environ.get("CFHD_AMD_HANDOFF"); os.environ["CFHD_AMD_HANDOFF"] = "host"
    try:
        text = refused(W, H, yuy2, 0, FILMSCAN2, N, 1, 1)
        assert text and "CFHD_AMD_HANDOFF" in text, text
        assert not refused(W, H, yuy2, 0, QUALITY_FILMSCAN1, N, 1, 1)
    finally:
        if old is None: os.environ.pop("CFHD_AMD_HANDOFF")
        else: os.environ["CFHD_AMD_HANDOFF"] = old


def gates_under_host_entropy():
    """Child process body (CFHD_AMD_ENTROPY=host is read when a batch is made; kept to a process of its own as tests/stream_batches.py does)."""
    for quality in (FILMSCAN2, QUALITY_FILMSCAN1):
        text = refused(W, H, FOURCCS["YUY2"], 0, quality, N, 1, 1)
        assert text and "CFHD_AMD_ENTROPY" in text, text
    print("HOST ENTROPY REFUSED")


def host_entropy_child(emulated):
    """Runs gates_under_host_entropy in a child process with CFHD_AMD_ENTROPY=host."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env["CFHD_AMD_ENTROPY"] = "host"
    code = "import sys; sys.path.insert(0, %r); import cfhd_testlib as T, group_stream_batches as S\n" % os.path.dirname(os.path.abspath(__file__))
    code += "with T.emulated_product(): S.gates_under_host_entropy()\n" if emulated else "S.gates_under_host_entropy()\n"
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "HOST ENTROPY REFUSED" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
