"""The antialiased cubic resize's reference (srcnn_resize_cubic_aa_*): the float64 formula include/srcnn_amd.h writes out, in
numpy and in the same order of operations -- torch.nn.functional.interpolate(mode="bicubic", align_corners=False,
antialias=True) -- and a float32 model of the two passes in the order the kernels sum.  Own code; nothing here calls the
library under test (model32 takes the tables as arguments: the tests hand it the library's own or this file's)."""
import functools

import numpy as np

A = -0.5

# Tolerance of a float32 result against ref64, as a multiple of max|x|: the bound the 4-tap float resize is documented to
# (tests/resize_f32_reference.py).  The float32 model below stays within 1.8e-7 on the shapes here.
TOL = 2e-6

# (sh, sw, dh, dw): the shapes the formula was checked on against torch -- /2.1, /2, /1.5, /3, /4.1, -> 1 x 1, the same size,
# x2, one axis only, 200 -> 13 and 9 -> 4
SHAPES = [(23, 29, 11, 13), (64, 96, 32, 48), (67, 131, 45, 87), (120, 90, 40, 30), (33, 33, 8, 8), (17, 19, 1, 1), (5, 7, 5, 7),
          (9, 11, 18, 22), (40, 50, 27, 50), (3, 200, 2, 13), (1, 9, 1, 4)]


def keys(x):
    x = np.abs(x)
    near = ((A + 2) * x - (A + 3)) * x * x + 1
    far = A * (((x - 5) * x + 8) * x - 4)
    return np.where(x < 1, near, np.where(x < 2, far, 0.0))


def taps64(s, n):
    """(first, count, coef) of one axis with s source and n output samples: int64 first and count, float64 coef (n, K) with K
    the largest count, zero beyond count[d]; every operation in the header's order (the sum of the weights sequential)."""
    rho = s / n
    m = rho if rho > 1.0 else 1.0
    support = 2.0 * m
    c = rho * (np.arange(n, dtype=np.float64) + 0.5)
    first = np.maximum(0, np.trunc(c - support + 0.5)).astype(np.int64)
    count = np.minimum(s, np.trunc(c + support + 0.5)).astype(np.int64) - first
    k = int(count.max())
    j = np.arange(k, dtype=np.int64)[None, :]
    w = keys(((j + first[:, None]).astype(np.float64) - c[:, None] + 0.5) / m)
    w = np.where(j < count[:, None], w, 0.0)
    total = np.cumsum(w, axis=1)[:, -1]             # sequential, ascending j (the padding adds exact zeros)
    w = np.where((total != 0.0)[:, None], w / np.where(total != 0.0, total, 1.0)[:, None], w)
    return first, count, w


def taps32(s, n):
    """taps64 with each coefficient rounded once to float32: what srcnn_cubic_aa_f32_taps returns."""
    first, count, w = taps64(s, n)
    return first.astype(np.int32), count.astype(np.int32), w.astype(np.float32)


def apply_axis(x, first, count, coef, dtype):
    """The last axis of x through a table, in `dtype`: acc = x_0 w_0, then acc = acc + x_j w_j for j ascending over exactly
    count[d] taps, every product and sum rounded to dtype."""
    x = np.asarray(x, dtype=dtype)
    coef = np.asarray(coef, dtype=dtype)
    s = x.shape[-1]
    acc = (x[..., first] * coef[:, 0]).astype(dtype)
    for j in range(1, coef.shape[1]):
        term = (x[..., np.minimum(first + j, s - 1)] * coef[:, j]).astype(dtype)
        acc = np.where(j < count, (acc + term).astype(dtype), acc)
    return acc


def resize(x, tx, ty, dtype):
    """Horizontal pass with table tx = (first, count, coef), then the vertical pass with ty, in dtype."""
    hor = apply_axis(x, *tx, dtype)
    return np.swapaxes(apply_axis(np.swapaxes(hor, -1, -2), *ty, dtype), -1, -2)


def ref64(x, dh, dw):
    """x (..., H, W) -> (..., dh, dw): the float64 formula."""
    sh, sw = np.shape(x)[-2:]
    return resize(x, taps64(sw, dw), taps64(sh, dh), np.float64)


def model32(x, tx, ty):
    """The kernels' float32 arithmetic on float32 tables (first, count, coef): bitwise what every kernel form returns."""
    return resize(np.asarray(x, dtype=np.float32), tx, ty, np.float32)


def uniform(shape, seed):
    """float32 uniform [0, 1) data of the given shape."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def torch64(x, dh, dw):
    """torch's own antialiased result on the CPU in float64."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).reshape((-1, 1) + np.shape(x)[-2:])
    y = F.interpolate(t, size=(dh, dw), mode="bicubic", align_corners=False, antialias=True)
    return y.numpy().reshape(np.shape(x)[:-2] + (dh, dw))


@functools.lru_cache(maxsize=None)
def case(sh, sw, dh, dw):
    """(x, ref64(x)) of one shape, computed once and shared: x float32 (sh, sw) uniform [0, 1).  Read-only."""
    x = uniform((sh, sw), 1000 * sh + sw + 7 * dh + dw)
    out = (x, ref64(x, dh, dw))
    for a in out:
        a.flags.writeable = False
    return out
