"""Every decoder output route -- sample kind x output format x resolution x scan x intra / two-frame group -- against the launches it makes, on the emulated product
library.

One child interpreter with HIPEMU_TRACE=1 decodes one 192x96 sample per row of ROWS through CFHD_PrepareToDecode / CFHD_DecodeSample; the emulator's launch trace
(tests/hipemu/hip/hip_runtime.h launch_sync) is the witness.  192x96 is the smallest size that passes every width rule at once: >= 128, whole six-pixel groups at full
and half width, a half width of whole 16-pixel blocks.  Per row the test asserts the two return codes and the exact sequence (kernel and grid) of the k_inv_* / k_half_* /
k_yu64_to_* / k_bayer_to_byr4 launches.  The decoder reads CFHD_AMD_INVERSE and CFHD_AMD_DEC_BLOCKS at every launch, so the rows switch them inside the one child.

EXPECTED was recorded (`python tests/test_output_routes_emulated.py record`) on the commit before the output route was gathered into one description
(cfhd_device.hip output_route), not from the code it now checks: what an output needs must not move when the code that decides it does.  The bytes of every route are
test_product_emulated.py's business; no reference library is needed here.

Test infrastructure only: nothing here is a product path."""
import ctypes, json, os, pprint, re, subprocess, sys
import numpy as np

W, H = 192, 96
GOP, INTERLACED, MATRIX_601 = 2, 1, 4      # encoding flags
TILE, STRIP = {"CFHD_AMD_INVERSE": "tile"}, {"CFHD_AMD_INVERSE": "strip"}
DENSE = dict(STRIP, CFHD_AMD_DEC_BLOCKS="0")
# sample kind: (input format, encoded format, encoding flags)
SAMPLES = {
    "422": ("YUY2", "422", 0), "422i": ("YUY2", "422", INTERLACED), "444": ("RG48", "444", 0), "4444": ("b64a", "4444", 0), "bayer": ("BYR4", "bayer", 0),
    "gop": ("YUY2", "422", GOP), "gopi": ("YUY2", "422", GOP | INTERLACED), "gop601": ("YUY2", "422", GOP | MATRIX_601),
}
FULL, HALF = 0, 1
# (sample kind, output format, resolution, environment)
ROWS = (
    [("422", f, FULL, {}) for f in ("YUY2", "2vuy", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a", "r210", "BYR4")] +
    [("422", "YUY2", FULL, e) for e in (TILE, STRIP, DENSE)] + [("422", "RG48", FULL, STRIP), ("422", "BGRA", FULL, STRIP)] +
    [("422", f, HALF, {}) for f in ("YUY2", "2vuy", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a", "r210")] +
    [("422i", f, FULL, {}) for f in ("YUY2", "2vuy", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a", "r210")] +
    [("422i", "YUY2", FULL, e) for e in (TILE, STRIP, DENSE)] + [("422i", "RG48", FULL, TILE), ("422i", "BGRA", FULL, TILE), ("422i", "b64a", FULL, STRIP)] +
    [("422i", f, HALF, {}) for f in ("YUY2", "YU64", "v210", "RG24", "BGRA", "RG48", "b64a")] +
    [("444", f, FULL, {}) for f in ("RG48", "b64a", "RG24", "BGRA", "BGRa", "r210", "DPX0", "AB10", "AR10", "YU64", "YUY2")] +
    [("444", "RG48", FULL, STRIP), ("444", "b64a", FULL, STRIP), ("444", "RG24", FULL, STRIP), ("444", "r210", FULL, STRIP)] +
    [("444", f, HALF, {}) for f in ("RG48", "b64a", "RG24", "BGRA", "BGRa", "r210", "AB10")] +
    [("4444", f, FULL, {}) for f in ("b64a", "RG48", "BGRA", "BGRa", "RG24", "r210")] + [("4444", "b64a", FULL, STRIP), ("4444", "RG48", FULL, STRIP)] +
    [("4444", f, HALF, {}) for f in ("b64a", "RG48", "BGRA", "BGRa", "RG24")] +
    [("bayer", "BYR4", FULL, {}), ("bayer", "BYR4", FULL, STRIP), ("bayer", "BYR4", HALF, {}), ("bayer", "RG48", FULL, {})] +
    [("gop", f, FULL, {}) for f in ("YUY2", "2vuy", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a", "r210")] +
    [("gop", f, HALF, {}) for f in ("YUY2", "2vuy", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a")] +
    [("gopi", f, FULL, {}) for f in ("YUY2", "YU64", "v210", "RG24", "BGRA", "BGRa", "RG48", "b64a")] + [("gopi", "RG48", FULL, TILE), ("gopi", "BGRA", FULL, TILE)] +
    [("gopi", f, HALF, {}) for f in ("YUY2", "YU64", "v210", "RG24", "BGRA", "RG48")] +
    [("gop601", f, FULL, {}) for f in ("YUY2", "v210", "RG24", "BGRA", "RG48", "b64a")] + [("gop601", "BGRA", HALF, {})]
)
DECODE = re.compile(r"k_(inv|half|yu64_to)_|k_bayer_to_byr4$")


def row_name(row):
    kind, fmt, half, env = row
    return " ".join([kind, fmt, "half" if half else "full"] + ["%s=%s" % (k.replace("CFHD_AMD_", "").lower(), v) for k, v in sorted(env.items())])


def _child():
    """Decodes every row; per row one 'ROW <name>' line on stderr ahead of its trace and one 'RC <name> <json>' line on stdout."""
    import cfhd_testlib as T
    with T.emulated_product() as L:
        samples = {}
        for kind, (fmt, enc, flags) in SAMPLES.items():
            frames = []
            for i in range(4 if flags & GOP else 1):
                if fmt == "YUY2": frame, pitch = T.synth_yuy2(W, H, 7 + i)
                elif fmt == "BYR4": frame, pitch = T.synth_bayer(W, H, 7 + i).reshape(-1).view(np.uint8).copy(), W * 2
                else:
                    words = {"RG48": 3, "b64a": 4}[fmt]
                    y, x = np.mgrid[0:H, 0:W * words]
                    frame, pitch = ((np.sin(x / 29.0 + i) * np.cos(y / 17.0) * 0.4 + 0.5) * 60000 + (x * y % 977)).astype(np.uint16).reshape(-1).view(np.uint8).copy(), W * words * 2
                frames.append(frame)
            encoded = {"422": T.ENCODED_YUV422, "444": T.ENCODED_RGB444, "4444": T.ENCODED_RGBA4444, "bayer": T.ENCODED_BAYER}[enc]
            out = T.amd_encode_frames(frames, pitch, W, H, T.fourcc(fmt), encoded=encoded, flags=flags)
            samples[kind] = out[1:3] if flags & GOP else out      # a group stream: sequence header, group, the P-frame header of its second frame, ...
        for row in ROWS:
            kind, fmt, half, env = row
            for k in ("CFHD_AMD_INVERSE", "CFHD_AMD_DEC_BLOCKS"): os.environ.pop(k, None)
            os.environ.update(env)
            os.write(2, ("ROW %s\n" % row_name(row)).encode())
            dec = ctypes.c_void_p(); assert L.CFHD_OpenDecoder(ctypes.byref(dec), None) == 0
            aw = ctypes.c_int(); ah = ctypes.c_int(); af = ctypes.c_uint32()
            first = samples[kind][0]
            sb = ctypes.create_string_buffer(first, len(first))
            rc = [L.CFHD_PrepareToDecode(dec, 0, 0, T.fourcc(fmt), 2 if half else 1, 0, sb, min(512, len(first)), ctypes.byref(aw), ctypes.byref(ah), ctypes.byref(af))]
            if rc[0] == 0:
                p = ctypes.c_int32(); assert L.CFHD_GetImagePitch(aw.value, af.value, ctypes.byref(p)) == 0
                for s in samples[kind]:
                    sb = ctypes.create_string_buffer(s, len(s)); out = np.zeros(p.value * ah.value, np.uint8)
                    rc.append(L.CFHD_DecodeSample(dec, sb, len(s), out.ctypes.data_as(ctypes.c_void_p), p.value))
            L.CFHD_CloseDecoder(dec)
            print("RC %s" % json.dumps([row_name(row), rc]), flush=True)


def observe():
    """row name -> [return codes (CFHD_PrepareToDecode, then CFHD_DecodeSample per sample), decode launches as 'kernel XxYxZ']"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFHD_AMD_")}
    env.update(HIPEMU_TRACE="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    seen, name = {}, None
    for line in run.stdout.splitlines():
        if line.startswith("RC "): name, rc = json.loads(line[3:]); seen[name] = [rc, []]
    for line in run.stderr.splitlines():
        if line.startswith("ROW "): name = line[4:]; continue
        m = re.match(r"\[hipemu\] (\S+?)(<.*>)?\s+grid (\d+) x (\d+) x (\d+) ", line)
        if not m or name is None: continue
        kernel = m.group(1).rsplit("::", 1)[-1]
        if DECODE.match(kernel): seen[name][1].append("%s %sx%sx%s" % (kernel, m.group(3), m.group(4), m.group(5)))
    return seen


EXPECTED = {'422 2vuy full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422 2x3x1']],
 '422 2vuy half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_yuv422 1x48x1']],
 '422 BGRA full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422_rgb32 2x3x1']],
 '422 BGRA full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422_rgb32 2x3x1']],
 '422 BGRA half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422 BGRa full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422_rgb32 2x3x1']],
 '422 BGRa half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422 BYR4 full': [[3], []],
 '422 RG24 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1', 'k_yu64_to_rgb24 1x96x1']],
 '422 RG24 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422 RG48 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1', 'k_yu64_to_rgb16 1x96x1']],
 '422 RG48 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1', 'k_yu64_to_rgb16 1x96x1']],
 '422 RG48 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422 YU64 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '422 YU64 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_yu64 1x48x1']],
 '422 YUY2 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422 2x3x1']],
 '422 YUY2 full dec_blocks=0 inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422_strip 1x3x1']],
 '422 YUY2 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422_strip_blocks 1x3x1']],
 '422 YUY2 full inverse=tile': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_yuv422 2x3x1']],
 '422 YUY2 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_yuv422 1x48x1']],
 '422 b64a full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1', 'k_yu64_to_rgb16 1x96x1']],
 '422 b64a half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422 r210 full': [[3], []],
 '422 r210 half': [[3], []],
 '422 v210 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1', 'k_yu64_to_v210 1x96x1']],
 '422 v210 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_yu64 1x48x1', 'k_yu64_to_v210 1x48x1']],
 '422i 2vuy full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_quad 1x48x1']],
 '422i BGRA full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_rows16 1x48x1', 'k_yu64_to_rgb16 1x96x1']],
 '422i BGRA full inverse=tile': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_rows16_col 1x48x1', 'k_yu64_to_rgb16 1x96x1']],
 '422i BGRA half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422i BGRa full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_rows16 1x48x1', 'k_yu64_to_rgb16 1x96x1']],
 '422i RG24 full': [[0, 3], []],
 '422i RG24 half': [[0, 3], []],
 '422i RG48 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_rows16 1x48x1', 'k_yu64_to_rgb16 1x96x1']],
 '422i RG48 full inverse=tile': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_rows16_col 1x48x1', 'k_yu64_to_rgb16 1x96x1']],
 '422i RG48 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422i YU64 full': [[0, 3], []],
 '422i YU64 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_yu64 1x48x1']],
 '422i YUY2 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_quad 1x48x1']],
 '422i YUY2 full dec_blocks=0 inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_strip 1x3x1']],
 '422i YUY2 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_strip_blocks 1x3x1']],
 '422i YUY2 full inverse=tile': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422 1x48x1']],
 '422i YUY2 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_yuv422 1x48x1']],
 '422i b64a full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_rows16 1x48x1', 'k_yu64_to_rgb16 1x96x1']],
 '422i b64a full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_frame_yuv422_rows16 1x48x1', 'k_yu64_to_rgb16 1x96x1']],
 '422i b64a half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb24 1x48x1']],
 '422i r210 full': [[3], []],
 '422i v210 full': [[0, 3], []],
 '422i v210 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_yu64 1x48x1', 'k_yu64_to_v210 1x48x1']],
 '444 AB10 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_rgb10 2x3x1']],
 '444 AB10 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb 1x48x1']],
 '444 AR10 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_rgb10 2x3x1']],
 '444 BGRA full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '444 BGRA half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb 1x48x1']],
 '444 BGRa full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '444 BGRa half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb 1x48x1']],
 '444 DPX0 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_rgb10 2x3x1']],
 '444 RG24 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '444 RG24 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '444 RG24 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb 1x48x1']],
 '444 RG48 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '444 RG48 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16_strip 1x1x1']],
 '444 RG48 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_packed16 1x48x1']],
 '444 YU64 full': [[3], []],
 '444 YUY2 full': [[3], []],
 '444 b64a full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '444 b64a full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_packed16 2x3x1']],
 '444 b64a half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb 1x48x1']],
 '444 r210 full': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_rgb10 2x3x1']],
 '444 r210 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_inv_rgb10 2x3x1']],
 '444 r210 half': [[0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x3', 'k_half_rgb 1x48x1']],
 '4444 BGRA full': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_inv_packed16 2x3x1']],
 '4444 BGRA half': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_half_rgb 1x48x1']],
 '4444 BGRa full': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_inv_packed16 2x3x1']],
 '4444 BGRa half': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_half_rgb 1x48x1']],
 '4444 RG24 full': [[3], []],
 '4444 RG24 half': [[3], []],
 '4444 RG48 full': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_inv_packed16 2x3x1']],
 '4444 RG48 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_inv_packed16_strip 1x1x1']],
 '4444 RG48 half': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_half_packed16 1x48x1']],
 '4444 b64a full': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_inv_packed16 2x3x1']],
 '4444 b64a full inverse=strip': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_inv_packed16_strip 1x1x1']],
 '4444 b64a half': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x2x4', 'k_half_packed16 1x48x1']],
 '4444 r210 full': [[3], []],
 'bayer BYR4 full': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x1x4', 'k_inv_packed16 1x2x1', 'k_bayer_to_byr4 1x48x1']],
 'bayer BYR4 full inverse=strip': [[0, 0], ['k_inv_plane 1x1x4', 'k_inv_plane 1x1x4', 'k_inv_packed16 1x2x1', 'k_bayer_to_byr4 1x48x1']],
 'bayer BYR4 half': [[3], []],
 'bayer RG48 full': [[3], []],
 'gop 2vuy full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_yuv422 2x3x2']],
 'gop 2vuy half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_yuv422 1x48x2']],
 'gop BGRA full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_yuv422_rgb32 2x3x2']],
 'gop BGRA half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gop BGRa full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_yuv422_rgb32 2x3x2']],
 'gop BGRa half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gop RG24 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_rgb24 1x96x2']],
 'gop RG24 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gop RG48 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_rgb16 1x96x2']],
 'gop RG48 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gop YU64 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2']],
 'gop YU64 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_yu64 1x48x2']],
 'gop YUY2 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_yuv422 2x3x2']],
 'gop YUY2 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_yuv422 1x48x2']],
 'gop b64a full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_rgb16 1x96x2']],
 'gop b64a half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gop r210 full': [[3], []],
 'gop v210 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_v210 1x96x2']],
 'gop v210 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_yu64 1x48x2', 'k_yu64_to_v210 1x48x2']],
 'gop601 BGRA full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_yuv422_rgb32 2x3x2']],
 'gop601 BGRA half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gop601 RG24 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_rgb24 1x96x1', 'k_yu64_to_rgb24 1x96x1']],
 'gop601 RG48 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_rgb16 1x96x1', 'k_yu64_to_rgb16 1x96x1']],
 'gop601 YUY2 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_yuv422 2x3x2']],
 'gop601 b64a full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_rgb16 1x96x1', 'k_yu64_to_rgb16 1x96x1']],
 'gop601 v210 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_packed16 2x3x2', 'k_yu64_to_v210 1x96x2']],
 'gopi BGRA full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_frame_yuv422_rows16 1x48x2', 'k_yu64_to_rgb16 1x96x2']],
 'gopi BGRA full inverse=tile': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_frame_yuv422_rows16_col 1x48x2', 'k_yu64_to_rgb16 1x96x2']],
 'gopi BGRA half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gopi BGRa full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_frame_yuv422_rows16 1x48x2', 'k_yu64_to_rgb16 1x96x2']],
 'gopi RG24 full': [[0, 3, 5], []],
 'gopi RG24 half': [[0, 3, 5], []],
 'gopi RG48 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_frame_yuv422_rows16 1x48x2', 'k_yu64_to_rgb16 1x96x2']],
 'gopi RG48 full inverse=tile': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_frame_yuv422_rows16_col 1x48x2', 'k_yu64_to_rgb16 1x96x2']],
 'gopi RG48 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_rgb24 1x48x2']],
 'gopi YU64 full': [[0, 3, 5], []],
 'gopi YU64 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_yu64 1x48x2']],
 'gopi YUY2 full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_frame_yuv422 1x48x2']],
 'gopi YUY2 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_yuv422 1x48x2']],
 'gopi b64a full': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_inv_frame_yuv422_rows16 1x48x2', 'k_yu64_to_rgb16 1x96x2']],
 'gopi v210 full': [[0, 3, 5], []],
 'gopi v210 half': [[0, 0, 0], ['k_inv_plane 1x1x3', 'k_inv_plane 1x2x6', 'k_half_yu64 1x48x2', 'k_yu64_to_v210 1x48x2']]}


def test_every_output_route_launches_what_it_launched_before():
    assert sorted(EXPECTED) == sorted(row_name(r) for r in ROWS), "ROWS and EXPECTED name different rows"
    seen = observe()
    wrong = ["%s:\n  expected %s\n  observed %s" % (n, EXPECTED[n], seen.get(n)) for n in sorted(EXPECTED) if seen.get(n) != EXPECTED[n]]
    assert not wrong, "\n".join(wrong)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "child": _child()
    else: pprint.pprint(observe(), width=250)
