"""MS-SSIM as srcnn_msssim_image_dev states it (include/srcnn_amd.h), in numpy float64, built on tests/metrics_reference.py:
the border shaved at scale 0, scale j + 1 the 2 x 2 mean of scale j with an odd last row or column paired with itself, and per
scale the sums of cs and ssim over the valid windows, each added exactly (math.fsum).  Nothing here imports the library."""
import math

import numpy as np

import metrics_reference as R

MAX_SCALES = 5
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli and Bovik 2003


def min_side(n_scales):
    return 10 * 2 ** (n_scales - 1) + 1


def reduce2(p):
    """((p(2y, 2x) + p(2y, 2x+1)) + (p(2y+1, 2x) + p(2y+1, 2x+1))) * 0.25, the index clamped at an odd end"""
    h, w = p.shape
    y0, x0 = np.arange(0, h, 2), np.arange(0, w, 2)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    return ((p[np.ix_(y0, x0)] + p[np.ix_(y0, x1)]) + (p[np.ix_(y1, x0)] + p[np.ix_(y1, x1)])) * 0.25


def pyramid(p, n_scales):
    """[scale 0 (the plane itself), ..., scale n_scales - 1]"""
    out = [np.asarray(p, np.float64)]
    for _ in range(n_scales - 1):
        out.append(reduce2(out[-1]))
    return out


def cs_ssim_maps(a, b, data_range):
    """(cs, ssim) per valid window; ssim is metrics_reference.ssim_map operation for operation"""
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ma, mb, eaa, ebb, eab = R.blur(a), R.blur(b), R.blur(a * a), R.blur(b * b), R.blur(a * b)
    mab = ma * mb
    cs_num = 2.0 * (eab - mab) + c2
    cs_den = ((eaa - ma * ma) + (ebb - mb * mb)) + c2
    num = (2.0 * mab + c1) * cs_num
    den = ((ma * ma + mb * mb) + c1) * cs_den
    return cs_num / cs_den, num / den


def msssim_plane(a, b, data_range, n_scales):
    """a, b: the REGION of one plane, float64 -> (n_scales, 3) {cs_sum, ssim_sum, n_win}"""
    assert 1 <= n_scales <= MAX_SCALES and min(a.shape) >= min_side(n_scales), (a.shape, n_scales)
    out = np.zeros((n_scales, 3))
    for s, (pa, pb) in enumerate(zip(pyramid(a, n_scales), pyramid(b, n_scales))):
        cs, ssim = cs_ssim_maps(pa, pb, data_range)
        out[s] = math.fsum(cs.ravel().tolist()), math.fsum(ssim.ravel().tolist()), float(cs.size)
    return out


def msssim_sums(a, b, border=0, luma=None, data_range=1.0, n_scales=5):
    """a, b: LOADED float64 arrays (C, H, W) -> (P, n_scales, 3)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and a.ndim == 3
    planes = [(R.luma_of(a, luma), R.luma_of(b, luma))] if luma is not None else list(zip(a, b))
    return np.stack([msssim_plane(R.shave(pa, border), R.shave(pb, border), data_range, n_scales) for pa, pb in planes])


def means(sums):
    """(..., S, 3) -> (..., S): cs_sum / n_win below the last scale, ssim_sum / n_win at it"""
    sums = np.asarray(sums, np.float64)
    top = np.arange(sums.shape[-2]) == sums.shape[-2] - 1
    return np.where(top, sums[..., 1], sums[..., 0]) / sums[..., 2]


def msssim_value(sums, weights=None):
    """prod max(mean_s, 0)^w_s; a mean that is not positive gives 0"""
    m = means(sums)
    w = np.asarray(WEIGHTS if weights is None else weights, np.float64)
    assert w.shape[-1] == m.shape[-1]
    with np.errstate(invalid="ignore"):
        return np.prod(np.where(m > 0, np.power(np.maximum(m, 0.0), w), 0.0), axis=-1)
