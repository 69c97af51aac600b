"""Hostile pictures for the GPU suite (tests/test_gpu_hostile.py) and their pin on the reference (tests/test_hostile_pictures_vs_ref.py): the inputs natural pictures
never give the kernels -- flat extremes (whole bands of zeros), noise on every byte (bands with no zero at all, saturating arithmetic), one-pixel stripes and
checkerboards (the largest highpass coefficients), single impulses in a flat frame (one listed block in an otherwise empty segment), steps.

A plain module: generators parametrised by width, height and format, the case lists, and `legal_for_reference`.

The reference encoder has no bound check on its sample buffer (w * h * bytes per pixel + 64 KB): a picture whose sample is larger makes it write past the buffer --
heap damage inside the test process.  So no test hands a picture to the reference before `legal_for_reference` holds for the sample the ORACLE + host writer
predict (their bytes equal the reference's on every legal case: test_hostile_pictures_vs_ref.py).  That is a condition on the inputs, asserted, not a skip."""
import numpy as np

NAMES = ("flat0", "flat128", "flat255", "noise", "bw", "vstripes", "hstripes", "checker", "impulses", "step")


def yuy2(name, w, h, fmt="YUY2"):
    """8-bit 4:2:2 picture `name` as an (h, 2 w) byte array; fmt "YUY2" (Y0 U Y1 V) or "2vuy" (U Y0 V Y1: the same picture, bytes of every pair exchanged)."""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:h, 0:w]
    if name.startswith("flat"): c = np.full((h, 2 * w), int(name[4:]), np.uint8)
    elif name == "noise": c = rng.integers(0, 256, (h, 2 * w), dtype=np.uint8)                                # uniform on every byte, chroma included
    elif name == "bw":                                                                                        # (behind the draw of the noise picture: the stream the measured sizes below were taken with)
        rng.integers(0, 256, (h, 2 * w), dtype=np.uint8); c = rng.choice(np.array([0, 255], np.uint8), (h, 2 * w))
    elif name == "vstripes": c = np.zeros((h, 2 * w), np.uint8); c[:, 0::4] = 255; c[:, 1::2] = 128           # luma 255, 0, ...; chroma 128
    elif name == "hstripes": c = np.full((h, 2 * w), 128, np.uint8); c[0::2, 0::2] = 255; c[1::2, 0::2] = 0   # luma rows 255 / 0
    elif name == "checker": c = np.full((h, 2 * w), 128, np.uint8); c[:, 0::2] = (((xx + yy) & 1) * 255).astype(np.uint8)
    elif name == "impulses": c = np.full((h, 2 * w), 128, np.uint8); c[0, 0] = 255; c[h - 1, 2 * w - 2] = 0; c[h // 2, w] = 255      # first pixel, last pixel, centre
    elif name == "step": c = np.zeros((h, 2 * w), np.uint8); c[:, w:] = 255                                   # left half 0, right half 255
    elif name.startswith("step_at"): c = np.full((h, 2 * w), 128, np.uint8); c[:, 0::2] = np.where(xx >= int(name[7:]), 255, 0).astype(np.uint8)      # luma 0 -> 255 at x
    elif name.startswith("impulses_at"):                                                                      # single luma impulses at x - 1 and x, rows apart, in flat 128
        x = int(name[11:]); c = np.full((h, 2 * w), 128, np.uint8); c[h // 4, 2 * (x - 1)] = 255; c[(3 * h) // 4, 2 * x] = 0
    else: raise KeyError(name)
    if fmt == "2vuy": c = c.reshape(h, w, 2)[:, :, ::-1].reshape(h, 2 * w)
    else: assert fmt == "YUY2"
    return np.ascontiguousarray(c)


def words16(name, rows, cols, channels=1):
    """The same shapes in 16-bit words, 0 / 65535 for the extremes: a (rows, cols * channels) array, every channel of a pixel alike except for the noise.
    RG48: channels 3, b64a: 4, a Bayer mosaic: 1 (rows x cols photosites)."""
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if name.startswith("flat"): p = np.full((rows, cols), {"0": 0, "128": 32768, "255": 65535}[name[4:]], np.uint16)
    elif name == "noise": return rng.integers(0, 65536, (rows, cols * channels), dtype=np.uint16)            # full range on every word
    elif name == "bw": return rng.choice(np.array([0, 65535], np.uint16), (rows, cols * channels))
    elif name == "vstripes": p = np.where(xx & 1, 0, 65535).astype(np.uint16)
    elif name == "hstripes": p = np.where(yy & 1, 0, 65535).astype(np.uint16)
    elif name == "checker": p = (((xx + yy) & 1) * 65535).astype(np.uint16)
    elif name == "impulses": p = np.full((rows, cols), 32768, np.uint16); p[0, 0] = 65535; p[rows - 1, cols - 1] = 0; p[rows // 2, cols // 2] = 65535
    elif name == "step": p = np.where(xx >= cols // 2, 65535, 0).astype(np.uint16)
    else: raise KeyError(name)
    return np.ascontiguousarray(np.repeat(p, channels, axis=1))


def b64a_checker_alternating_alpha(w, h):
    """b64a words A, R, G, B: colour checkerboard 0 / 65535, alpha 65535 / 0 from pixel to pixel."""
    px = words16("checker", h, w, 4)
    px[:, 0::4] = np.where((np.arange(w) & 1)[None, :], 0, 65535)
    return px


def legal_for_reference(want_sample, w, h, bytes_per_pixel):
    """True only when the sample the oracle + host writer predict fits w * h * bytes_per_pixel bytes: the reference's buffer less its whole 64 KB padding."""
    return len(want_sample) <= w * h * bytes_per_pixel


# 4:2:2 intra cases at 336 x 252 (tiled kernels, pad rows 252 -> 256, odd lowpass widths): every picture at quality 1 (LOW), every picture but the two kinds of noise at
# quality 4 (FILMSCAN1).
YUY2_CASES = [(n, q) for q in (4, 1) for n in NAMES if not (q == 4 and n in ("noise", "bw"))]
"""Sample sizes of the reference (== oracle + host writer, byte for byte) in bytes, 8-bit YUY2; the reference's buffer is w * h * 2 + 65536, legal is <= w * h * 2.

    336 x 252 (buffer 234 880, legal up to 169 344)      FILMSCAN1 (4)    LOW (1)
      flat 0 / 128 / 255                                  11 564 / 9 176 / 11 564     10 484 / 9 176 / 10 484
      noise                                               244 328  ILLEGAL            141 832
      bw (random 0 / 255)                                 283 836  ILLEGAL            170 004 (*)
      vstripes / hstripes                                 62 488 / 61 988             38 364 / 38 176
      checker / impulses / step                           54 052 / 9 340 / 15 828     35 528 / 9 260 / 13 780
    2048 x 72 (buffer 360 448, legal up to 294 912)
      flat 0 / 128 / 255                                  13 580 each                 13 580 each
      noise / bw                                          420 424 / 487 696 ILLEGAL   242 696 / 290 680
      stripes (both) / checker / impulses / step          105 552 / 91 728 / 13 708 / 14 692      64 080 / 59 472 / 13 652 / 14 432

(*) 660 bytes above the legal bound (inside the 64 KB padding, so the reference itself is safe): by the rule the case is not legal, and the quality-1 list leaves it to
the oversize tests, which never call the reference."""
YUY2_CASES.remove(("bw", 1))
# The PSNR witness of test_gpu_parity._check_decode (the product's PSNR within 0.1 dB of the reference decoder's) compares two random dithers.  With m bytes the dither can
# move by one step in a picture that is otherwise exact, the mean squared error is a sum of m coin flips: two dithers differ by about 4.34 * sqrt(2 / m) dB (one sigma).
# Measured: the FILMSCAN1 sample of the vertical stripes has m = 168 of 169 344 bytes, lies between 78.2 dB (all moved) and 99 dB (none), and two runs of the reference
# decoder on it gave 81.44 and 82.64 dB; flat 255 differed by 0.23 dB from run to run.  Three sigma below 0.1 dB needs m > 2 * (3 * 4.34 / 0.1) ** 2 = 33 900: below
# that the witness is the reference's rand() and nothing else, and a case is decoded without it (every other check of _check_decode holds, the reference's picture
# must lie in the interval too).
PSNR_WITNESS_MIN_MOVABLE = 34000

# the batched strip path at 2048 x 72 (two segments: 1984 pixels + a partial one), FILMSCAN1: everything legal there, plus two pictures made for the segment boundary
STRIP_W, STRIP_H = 2048, 72
STRIP_CASES = [n for n in NAMES if n not in ("noise", "bw")] + ["step_at1984", "impulses_at1984"]
# oversize at 336 x 252, FILMSCAN1: the reference would overrun its buffer; the product answers CFHD_ERROR_CODEC_ERROR
OVERSIZE = ("noise", "bw")

FAMILY_CASES = ("RG48 checker", "RG48 noise", "b64a checker + alternating alpha", "BYR4 checker", "interlaced hstripes", "group flat0, flat255", "group flat255, flat0")
"""One shape per other transform family, all at FILMSCAN1.  Sample sizes of the reference (== oracle + host writer, byte for byte; measured with the reference on the CPU,
pinned in test_hostile_pictures_vs_ref.py) beside the reference's buffer (w * h * bytes per pixel + 65536) and the legal bound (w * h * bytes per pixel):

    RG48 -> RGB 4:4:4, 320 x 240 (buffer 526 336, legal 460 800)       checker 114 088     noise 298 388 (quality 3: 264 640, 2: 211 556, 1: 166 424 -- FILMSCAN1 is legal)
    b64a -> RGBA 4:4:4:4, 320 x 240 (buffer 679 936, legal 614 400)    checker + alternating alpha 148 680
    BYR4 -> Bayer, 192 x 96 (buffer 102 400, legal 36 864)             checker mosaic 4 264
    interlaced YUY2, 320 x 64 (buffer 106 496, legal 40 960)           rows 255 / 0: 4 596
    two-frame group YUY2, 320 x 240 (buffer 219 136, legal 153 600)    flat 0 then flat 255, and the reverse: sequence header 40, group 30 092"""
FAMILY_SIZES = {"RG48 checker": 114088, "RG48 noise": 298388, "b64a": 148680, "BYR4": 4264, "interlaced": 4596, "group": 30092}
