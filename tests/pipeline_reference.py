"""Helpers of the resize / colour edge tests (tests/test_resize_geometry_cpu.py, tests/test_gpu_pipeline_edges.py) -- TEST
INFRASTRUCTURE, built on the oracle alone, nothing of the product.

cv::resize(INTER_CUBIC) on x86 runs its vertical pass in float32 for the columns below dw - dw % 8 and in fixed point for the
last dw % 8 columns (oracle/opencv_steps.c).  On ordinary pictures the two passes disagree in about one pixel in 10^5, so a
kernel that put the split in the wrong place would pass a test on such pictures.  This module restates the resize in numpy with
BOTH passes for every column, builds planes on which the passes disagree in whole rows (tie_plane), and counts where they do
(discriminating), so that a test can say from the reference alone that its input tells the two passes apart."""
import numpy as np

import oracle

DIRECT, TILED, TILED4 = 0, 1, 2


def resize_both(src, dw, dh):
    """-> (fixed, flt): the cubic resize of one 8-bit plane with the fixed-point vertical pass (sum + 2^21) >> 22 for EVERY
    column, and with the float32 pass (every product and every sum rounded on its own, in OpenCV's order, then nearest-even
    and saturate) for every column."""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    xofs, alpha = oracle.cubic_table(sw, dw)
    yofs, beta = oracle.cubic_table(sh, dh)
    k = np.arange(4)
    xi = np.clip(xofs[:, None] - 1 + k, 0, sw - 1)                                  # [dw, 4]
    yi = np.clip(yofs[:, None] - 1 + k, 0, sh - 1)                                  # [dh, 4]
    hsum = (src.astype(np.int64)[:, xi] * alpha.astype(np.int64)).sum(axis=2)       # [sh, dw], the horizontal pass
    taps = hsum[yi]                                                                 # [dh, 4, dw]
    fixed = ((taps * beta.astype(np.int64)[:, :, None]).sum(axis=1) + (1 << 21)) >> 22
    b = beta.astype(np.float32) * (np.float32(1) / np.float32(2048 * 2048))         # [dh, 4], float32
    t = taps.astype(np.float32)                                                     # exact: |sum| < 2^24
    r = t[:, 3] * b[:, 3, None]
    for j in (2, 1, 0):
        r = t[:, j] * b[:, j, None] + r                                             # two ufuncs: product and sum both rounded
    assert r.dtype == np.float32
    return np.clip(fixed, 0, 255).astype(np.uint8), np.clip(np.rint(r), 0, 255).astype(np.uint8)


def split_column(dw):
    return dw - dw % 8


def resize_record(src, dw, dh):
    """The variant of record (oracle.VERTICAL_SIMD_FLOAT) from the two passes: float below the split, fixed from it on."""
    fixed, flt = resize_both(src, dw, dh)
    out = flt.copy()
    out[:, split_column(dw):] = fixed[:, split_column(dw):]
    return out


def tie_plane(sw, sh, phase):
    """Constant along every row, g(y) = (y + phase) // 2 mod 256.  Where an output row has vertical phase exactly 1/2 its
    coefficients are (-128, 1152, 1152, -128); where its four taps read (v, v, v + 1, v + 1) the sum is exactly v + 1/2: the
    fixed pass gives v + 1, the float pass v when v is even -- in every column whose four horizontal coefficients sum to 2048."""
    g = ((np.arange(sh) + phase) // 2) % 256
    return np.repeat(g[:, None], sw, axis=1).astype(np.uint8)


def tie_phase(sh, dh):
    """The phase of tie_plane at which the rows of vertical phase 1/2 read (v, v, v + 1, v + 1): 0 at x1.25, else 1
    (x1.5, x2.5, 2:1 down).  x2 and x3 have no row of phase 1/2."""
    return 0 if 4 * dh == 5 * sh else 1


def discriminating(src, dw, dh):
    """-> (pixels with fixed != flt in the 8 columns below the split, pixels with fixed != flt in the tail columns)."""
    fixed, flt = resize_both(src, dw, dh)
    d = fixed != flt
    s = split_column(dw)
    return int(d[:, max(s - 8, 0):s].sum()), int(d[:, s:].sum())


def visible_step(src, dw, dh):
    """Output rows of a row-constant plane in which the variant of record steps at the split: among the columns whose
    horizontal coefficients sum to 2048 (the others do not tie) every one of the 8 columns below the split holds u, every tail
    column u + 1, for one u.  -> number of such rows."""
    rec = oracle.resize_cubic(src, dw, dh).astype(int)
    _, alpha = oracle.cubic_table(np.asarray(src).shape[1], dw)
    full = alpha.astype(int).sum(axis=1) == 2048
    s = split_column(dw)
    below = [c for c in range(max(s - 8, 0), s) if full[c]]
    tail = [c for c in range(s, dw) if full[c]]
    if not below or not tail:
        return 0
    lo, hi = rec[:, below], rec[:, tail]
    rows = (lo.min(axis=1) == lo.max(axis=1)) & (hi.min(axis=1) == hi.max(axis=1)) & (hi[:, 0] == lo[:, 0] + 1)
    return int(rows.sum())


# (sw, sh, dw, dh, expected kernel, wants_tie).  The expected kernel is written down by hand from the documented limits
# (the pipeline kernels): tiled4 needs ceil(32 sh / dh) + 4 <= 28, ceil(256 sw / dw) + 5 <= 288 and dw % 4 == 0,
# tiled ceil(8 sh / dh) + 4 <= 16 and the same column limit.
SHAPES = [
    (168, 200, 252, 300, TILED4, True),     # dw % 8 = 4, 9 row tiles + 12 rows, x1.5
    (344, 90, 516, 135, TILED4, True),      # last column tile = 4 px, all of it tail; last row tile 7 rows
    (40, 64, 60, 96, TILED4, True),         # one small tile with a tail
    (40, 96, 60, 128, TILED4, False),       # sh / dh = 0.75: row span 28 = RMAX4 exactly
    (40, 97, 60, 128, TILED, False),        # one source row past the tiled4 limit
    (283, 48, 256, 64, TILED4, False),      # column span 288 = SMAX exactly
    (283, 48, 260, 64, TILED4, False),      # the same with a tail and a 4-px last column tile
    (284, 48, 256, 64, DIRECT, False),      # one source column past SMAX
    (64, 96, 100, 64, TILED, False),        # sh / dh = 1.5: row span 16 = RMAX exactly
    (64, 97, 100, 64, DIRECT, False),       # one past
    (48, 100, 60, 125, TILED, True),        # x1.25 (phase 0)
    (49, 100, 61, 125, TILED, True),        # dw % 8 = 5
    (200, 120, 100, 60, DIRECT, True),      # 2:1 down: every column ties
    (96, 20, 60, 200, DIRECT, False),       # down in x, x10 in y
    (20, 96, 200, 60, DIRECT, False),       # x10 in x, down in y
    (1, 1, 300, 40, TILED4, False),         # all taps clamped, two column tiles
    (2, 1000, 8, 1500, TILED4, False),      # 47 row tiles of a 2-px source
    (40, 30, 320, 240, TILED4, False),      # x8
    (600, 40, 780, 60, TILED4, False),      # 4 column tiles, dw % 8 = 4
    (1, 7, 1, 9, TILED, False),             # dw < 8: all tail
    (7, 1, 12, 1, TILED, False),            # dw % 4 == 0 but sh / dh = 1
    (300, 7, 400, 7, TILED, False),         # x1.33 in x only
]

# The whole-pipeline cases of tests/test_gpu_pipeline_edges.py: (w, h, scale, (ow, oh), takes the two fused launches).
# The fused launches need the tiled4 limits and dword-aligned rows (ow % 4 == 0); every fused case here has ow % 8 == 4.
PIPELINE_CASES = [
    (40, 64, 1.5, (60, 96), True),
    (168, 100, 1.5, (252, 150), True),
    (344, 90, 1.5, (516, 135), True),
    (80, 60, 1.35, (108, 81), True),        # ceil(32 * 60 / 81) + 4 = 28: at the tiled4 row limit
    (90, 50, 2.0, (180, 100), True),
    (80, 60, 1.3, (104, 78), False),        # ceil(32 * 60 / 78) + 4 = 29: one past it, the three separate kernels
    (41, 64, 1.5, (61, 96), False),         # ow % 4 != 0
]


def chroma_tie_image(w, h, comp):
    """B, G, R image whose Cr (comp = 1) or Cb (comp = 2) plane is 100 + (y + 1) // 2 in row y: tie_plane(w, h, 1) + 100, the
    other two channels fixed at 100 and R (Cr) or B (Cb) chosen per row through the oracle's own conversion."""
    ramp = np.full((256, 1, 3), 100, np.uint8)
    ramp[:, 0, 2 if comp == 1 else 0] = np.arange(256)
    plane = oracle.bgr2ycrcb(ramp)[comp][:, 0].astype(int)
    img = np.full((h, w, 3), 100, np.uint8)
    for y in range(h):
        hit = np.flatnonzero(plane == 100 + (y + 1) // 2)
        assert hit.size, f"no byte gives component value {100 + (y + 1) // 2}"
        img[y, :, 2 if comp == 1 else 0] = hit[0]
    return img
