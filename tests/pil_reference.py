"""Pillow's 8-bit two-pass resize (Image.resize of a uint8 picture with BILINEAR or BICUBIC), restated in numpy.

The arithmetic of include/srcnn_amd.h ("Pillow's resize of uint8 images"), operation for operation: float64 coefficients
in the order written there, integer coefficients with 22 fractional bits, int32 sums, a rounded and saturated uint8 after the
horizontal pass and again after the vertical one.  tests/test_pil_cpu.py holds it to Pillow itself byte for byte; the GPU tests
hold the kernels to it.

SHAPES is the list every test walks: (src_h, src_w, dst_h, dst_w).  tile_bounds() reads the tile sizes of the kernels from
srcnn_image.h, and bound_shapes() makes destination sizes of bound - 1, bound, bound + 1 from them.
"""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
BILINEAR, BICUBIC = 2, 3                  # Pillow's own numbers (Image.Resampling)
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC}
PRECISION_BITS = 22

SHAPES = [
    (23, 37, 46, 74), (23, 37, 69, 111), (23, 37, 35, 55), (61, 97, 30, 48), (61, 97, 20, 32), (61, 97, 14, 23),
    (9, 200, 9, 13),        # the height is kept: no vertical pass; up to 62 taps (Pillow's ksize is 63): the general form
    (40, 31, 1, 1), (1, 1, 5, 5), (5, 7, 5, 14), (5, 7, 10, 7), (17, 19, 17, 19), (2, 3, 7, 8), (64, 64, 129, 127),
    (33, 65, 16, 257),
]
# the tile bounds the kernels had when the list below was written: PIL_TR output rows and PIL_TC output columns per workgroup of
# the tiled form, PIL_HC output columns per workgroup of the general form's two launches
EXPECTED_BOUNDS = {"PIL_TR": 16, "PIL_TC": 64, "PIL_HC": 256}
BOUND_SHAPES = [
    # rows around PIL_TR, columns around PIL_TC (tiled form: ratios within 4)
    (11, 40, 15, 63), (11, 40, 16, 64), (11, 40, 17, 65),
    # columns around PIL_HC; the 5 : 1 shrink of the rows sends these to the general form
    (85, 130, 17, 255), (80, 130, 16, 256), (75, 130, 15, 257),
]


def tile_bounds():
    """{name: value} of the PIL_* tile constants as srcnn_cpp_amd/csrc/srcnn_image.h declares them"""
    text = (ROOT / "srcnn_cpp_amd" / "csrc" / "srcnn_image.h").read_text()
    out = {}
    for name in EXPECTED_BOUNDS:
        m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", text)
        if m is None:
            raise AssertionError(f"srcnn_image.h declares no {name}")
        out[name] = int(m.group(1))
    return out


def bound_shapes(bounds=None):
    """Destination sizes of bound - 1, bound, bound + 1 for every tile bound, made from the bounds themselves"""
    b = bounds or tile_bounds()
    tr, tc, hc = b["PIL_TR"], b["PIL_TC"], b["PIL_HC"]
    out = [(11, 40, tr + k, tc + k) for k in (-1, 0, 1)]
    out += [(5 * (tr - k), 130, tr - k, hc + k) for k in (-1, 0, 1)]
    return out


def all_shapes():
    return SHAPES + BOUND_SHAPES


def _kernel(filt, x):
    x = np.abs(x)
    if filt == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def taps(src_n, dst_n, filt):
    """One axis: (first[dst_n], count[dst_n], coef[dst_n][kmax] int32, zero beyond count) -- precompute_coeffs and
    normalize_coeffs_8bpc of Pillow's Resample.c"""
    if filt not in (BILINEAR, BICUBIC):
        raise ValueError(f"filter {filt}")
    support_unit = 1.0 if filt == BILINEAR else 2.0
    scale = float(src_n) / float(dst_n)
    fs = 1.0 if scale < 1.0 else scale
    support = support_unit * fs
    ss = 1.0 / fs
    d = np.arange(dst_n, dtype=np.float64)
    center = (d + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # astype truncates toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), src_n)
    count = xmax - xmin
    kmax = int(count.max())
    j = np.arange(kmax, dtype=np.int64)[None, :]
    w = _kernel(filt, ((j + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where(j < count[:, None], w, 0.0)
    ww = w[:, 0].copy()
    for k in range(1, kmax):              # ((w_0 + w_1) + w_2) + ...; the zeros beyond count add nothing
        ww = ww + w[:, k]
    safe = np.where(ww != 0.0, ww, 1.0)
    w = np.where((ww != 0.0)[:, None], w / safe[:, None], w)
    scaled = w * float(1 << PRECISION_BITS)
    coef = np.where(w < 0.0, (-0.5 + scaled).astype(np.int64), (0.5 + scaled).astype(np.int64))
    coef = np.where(j < count[:, None], coef, 0)
    return xmin.astype(np.int32), count.astype(np.int32), coef.astype(np.int32)


def _pass_sums(a, first, count, coef):
    """The int64 sums (1 << 21) + sum_j a[..., first + j] * coef_j along the LAST axis of a (any integer or float array)"""
    n = first.shape[0]
    j = np.arange(coef.shape[1])[None, :]
    idx = np.minimum(first[:, None].astype(np.int64) + j, a.shape[-1] - 1)      # (beyond count: coefficient 0)
    g = a[..., idx]                                                             # [..., n, kmax]
    if np.issubdtype(a.dtype, np.floating):
        return (g * coef.astype(np.float64)).sum(axis=-1) + float(1 << (PRECISION_BITS - 1))
    acc = (g.astype(np.int64) * coef.astype(np.int64)).sum(axis=-1) + (1 << (PRECISION_BITS - 1))
    assert np.abs(acc).max() < 2 ** 31, "the int32 accumulator of a pass would overflow"
    assert n == acc.shape[-1]
    return acc


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, dst_h, dst_w, filt=BICUBIC, wrong=None):
    """img: uint8 (H, W) or (H, W, C) -> uint8 (dst_h, dst_w[, C]).  wrong: None for Pillow's arithmetic; "unrounded" keeps the
    horizontal results unrounded between the passes, "vertical_first" runs the vertical pass first -- the two mistakes the
    bitwise tests must catch."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    planes = img[None] if img.ndim == 2 else np.moveaxis(img, 2, 0)            # [C, H, W]
    src_h, src_w = planes.shape[1:]
    need_h, need_v = dst_w != src_w, dst_h != src_h

    def horizontal(p):
        return _pass_sums(p, *taps(src_w, dst_w, filt))

    def vertical(p):
        return np.swapaxes(_pass_sums(np.swapaxes(p, 1, 2), *taps(src_h, dst_h, filt)), 1, 2)

    out = planes
    if wrong == "vertical_first":
        if need_v:
            out = _clip8(vertical(out))
        if need_h:
            out = _clip8(horizontal(out))
    elif wrong == "unrounded":
        if need_h and need_v:
            mid = (horizontal(out).astype(np.float64) - float(1 << (PRECISION_BITS - 1))) / float(1 << PRECISION_BITS)
            acc = np.floor(vertical(mid)).astype(np.int64)
            out = _clip8(acc)
        elif need_h:
            out = _clip8(horizontal(out))
        elif need_v:
            out = _clip8(vertical(out))
    else:
        assert wrong is None
        if need_h:
            out = _clip8(horizontal(out))
        if need_v:
            out = _clip8(vertical(out))
    out = np.ascontiguousarray(out)
    return out[0] if img.ndim == 2 else np.ascontiguousarray(np.moveaxis(out, 0, 2))


def inputs(src_h, src_w, seed=0):
    """The three inputs of a shape: random bytes (H, W), a period-1 checkerboard of 0 / 255 (H, W), and H x W x 3 draws from
    {0, 1, 128, 254, 255}"""
    rng = np.random.default_rng([seed, src_h, src_w])
    yy, xx = np.mgrid[0:src_h, 0:src_w]
    return {
        "random": rng.integers(0, 256, (src_h, src_w), dtype=np.uint8),
        "checker": (((yy + xx) & 1) * 255).astype(np.uint8),
        "extremes": rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), size=(src_h, src_w, 3)),
    }
