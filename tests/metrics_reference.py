"""The metrics of srcnn_metrics_image_dev (include/srcnn_amd.h) stated in numpy float64: load, luma, shave, SSE, separable SSIM.
Nothing here imports the library.  Arrays are (C, H, W) or (H, W); a loaded value is a float32 widened to float64."""
import math

import numpy as np

WIN = 11
LUMA_BT601 = (0.299, 0.587, 0.114, 0.0)


def window():
    """g[i] = exp(-(i - 5)^2 / 4.5) / sum, float64"""
    g = np.array([math.exp(-((i - 5) ** 2) / 4.5) for i in range(WIN)], np.float64)
    return g / g.sum()


def load(x, scale=None):
    """The load rule: float32 as it is, float16 widened exactly, uint8 as (float32)b * (float32)scale; then float64.  (bfloat16
    has no numpy type: the tests hand over the float32 the bits widen to.)"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return (x.astype(np.float32) * np.float32(1.0 / 255.0 if scale is None else scale)).astype(np.float64)
    if x.dtype in (np.float32, np.float16):
        return x.astype(np.float32).astype(np.float64)
    raise TypeError(x.dtype)


def luma_of(x3, luma):
    """((w0 c0 + w1 c1) + w2 c2) + offset in float64 from the float32 weights; x3: loaded (3, H, W)"""
    w = np.asarray(luma, np.float32).astype(np.float64)
    return ((w[0] * x3[0] + w[1] * x3[1]) + w[2] * x3[2]) + w[3]


def shave(p, border):
    return p[border:p.shape[0] - border, border:p.shape[1] - border] if border else p


def sse_plane(a, b):
    """sum (a - b)^2, the float64 terms added exactly (math.fsum): one rounding, so that a bound on the kernel's sum is a bound
    against this"""
    d = a - b
    return math.fsum((d * d).ravel().tolist()), float(a.size)


def _valid(p, g, axis):
    n = p.shape[axis] - (WIN - 1)
    idx = [slice(None)] * 2
    out = 0.0
    for j in range(WIN):
        idx[axis] = slice(j, j + n)
        out = out + g[j] * p[tuple(idx)]
    return out


def blur(p):
    g = window()
    return _valid(_valid(p, g, 0), g, 1)


def ssim_map(a, b, data_range):
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ma, mb, eaa, ebb, eab = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
    mab = ma * mb
    num = (2.0 * mab + c1) * (2.0 * (eab - mab) + c2)
    den = ((ma * ma + mb * mb) + c1) * (((eaa - ma * ma) + (ebb - mb * mb)) + c2)
    return num / den


def ssim_plane(a, b, data_range):
    m = ssim_map(a, b, data_range)
    return math.fsum(m.ravel().tolist()), float(m.size)


def ssim_map_direct(a, b, data_range):
    """The definition evaluated window by window with the 2-D window g g^T: no separable pass"""
    g2 = np.outer(window(), window())
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    h, w = a.shape[0] - 10, a.shape[1] - 10
    out = np.empty((h, w))
    for y in range(h):
        for x in range(w):
            pa, pb = a[y:y + WIN, x:x + WIN], b[y:y + WIN, x:x + WIN]
            ma, mb = (g2 * pa).sum(), (g2 * pb).sum()
            eaa, ebb, eab = (g2 * pa * pa).sum(), (g2 * pb * pb).sum(), (g2 * pa * pb).sum()
            out[y, x] = ((2 * ma * mb + c1) * (2 * (eab - ma * mb) + c2)) / ((ma * ma + mb * mb + c1) * ((eaa - ma * ma) + (ebb - mb * mb) + c2))
    return out


def metrics(a, b, border=0, luma=None, data_range=1.0, ssim=True, sse=True):
    """a, b: LOADED float64 arrays (C, H, W) -> (P, 4) float64 {sse, n_px, ssim_sum, n_win}; the fields of a metric that was
    not asked for are 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and a.ndim == 3
    planes = [(luma_of(a, luma), luma_of(b, luma))] if luma is not None else list(zip(a, b))
    out = np.zeros((len(planes), 4))
    for k, (pa, pb) in enumerate(planes):
        pa, pb = shave(pa, border), shave(pb, border)
        if sse:
            out[k, 0], out[k, 1] = sse_plane(pa, pb)
        if ssim:
            out[k, 2], out[k, 3] = ssim_plane(pa, pb, data_range)
    return out


def _valid_last(p, g, axis):
    """_valid along axis -2 or -1 of an array with any leading dimensions: the same products and sums in the same order"""
    n = p.shape[axis] - (WIN - 1)
    out = 0.0
    for j in range(WIN):
        idx = (Ellipsis, slice(j, j + n)) if axis == -1 else (Ellipsis, slice(j, j + n), slice(None))
        out = out + g[j] * p[idx]
    return out


def _fsum_rows(x):
    """math.fsum of every plane of x (..., H, W) -> (...)"""
    flat = x.reshape(-1, x.shape[-2] * x.shape[-1])
    return np.array([math.fsum(r) for r in flat.tolist()]).reshape(x.shape[:-2])


def metrics_batch(a, b, border=0, luma=None, data_range=1.0, ssim=True, sse=True):
    """metrics() of every frame of a, b: LOADED float64 arrays (N, C, H, W) -> (N, P, 4), the element-wise arithmetic done on
    all planes at once.  Every value goes through the operations of metrics() in their order and every plane's sum is the same
    math.fsum, so the result is metrics() of each frame (tests/test_metrics_cpu.py holds it to that)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and a.ndim == 4
    if luma is not None:
        w = np.asarray(luma, np.float32).astype(np.float64)
        a, b = ((((w[0] * x[:, 0] + w[1] * x[:, 1]) + w[2] * x[:, 2]) + w[3])[:, None] for x in (a, b))
    if border:
        a, b = (x[..., border:x.shape[-2] - border, border:x.shape[-1] - border] for x in (a, b))
    out = np.zeros(a.shape[:2] + (4,))
    if sse:
        d = a - b
        out[..., 0], out[..., 1] = _fsum_rows(d * d), float(a.shape[-2] * a.shape[-1])
    if ssim:
        g = window()
        blur_nd = lambda p: _valid_last(_valid_last(p, g, -2), g, -1)
        c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
        ma, mb, eaa, ebb, eab = blur_nd(a), blur_nd(b), blur_nd(a * a), blur_nd(b * b), blur_nd(a * b)
        mab = ma * mb
        num = (2.0 * mab + c1) * (2.0 * (eab - mab) + c2)
        den = ((ma * ma + mb * mb) + c1) * (((eaa - ma * ma) + (ebb - mb * mb)) + c2)
        m = num / den
        out[..., 2], out[..., 3] = _fsum_rows(m), float(m.shape[-2] * m.shape[-1])
    return out


def periodic_rows(block, rows):
    """`rows` rows of a picture whose rows repeat `block` (B, W) with period B"""
    reps = -(-rows // block.shape[0])
    return np.tile(block, (reps, 1))[:rows]


def sse_bound(n_px):
    """relative error of a float64 sum of n non-negative terms, each exact to 2 roundings, in any order"""
    return (n_px + 4) * 2.0 ** -53


SSIM_TOL = 1e-9      # |ssim_sum / n_win - reference| for data in [0, L]: a few dozen roundings of 2^-53 on quantities <= 2 L^2 against C1 = 1e-4 L^2


# ---- data ----------------------------------------------------------------------------------------------------------------
def noise(shape, seed, L=1.0):
    return (np.random.default_rng(seed).random(shape) * L).astype(np.float32)


def smooth(shape, seed, L=1.0):
    """a smooth field plus small noise, in [0, L]"""
    h, w = shape[-2:]
    yy, xx = np.mgrid[0:h, 0:w]
    f = 0.5 + 0.35 * np.sin(yy / 7.0 + seed) * np.cos(xx / 5.0) + 0.02 * np.random.default_rng(seed).standard_normal(shape)
    return (np.clip(f, 0.0, 1.0) * L).astype(np.float32)


def near_constant(shape, L=1.0):
    """0.999 L everywhere; the second picture differs in one pixel: where E[x^2] - mu^2 cancels in float32"""
    a = np.full(shape, 0.999 * L, np.float32)
    b = a.copy()
    b[..., shape[-2] // 2, shape[-1] // 2] = np.float32(0.5 * L)
    return a, b
