"""The float32 cubic resize's reference: a float64 numpy restatement of the arithmetic include/srcnn_amd.h fixes for
srcnn_resize_cubic_f32 -- torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=False) with the
coordinates in float64 -- plus the tolerance and the shapes the CPU and GPU tests share.  Own code; nothing here calls the
library under test."""
import functools

import numpy as np

A = -0.75

# Tolerance of a float32 result against ref64, as a multiple of max|x|: at most about 12 float32 roundings of relative size
# 2^-24 (four coefficient roundings, four products and three sums per pass, two passes, the later ones acting on fewer terms),
# each on sums of absolute terms <= (1.375)^2 max|x| (1.375 = the largest sum of |coefficients|, at t = 1/2):
# 12 * 2^-24 * 1.89 = 1.4e-6.
TOL = 2e-6

# (sh, sw, dh, dw) of the GPU tests' accuracy cases.  The first three clamp every tap; 511 and 900 columns cross output column
# 256 and span several column tiles; the last is far outside any tile span (the direct form), 23x29 -> 11x13 a mild down-scale.
CASES = [(1, 1, 3, 5), (2, 3, 5, 7), (5, 4, 10, 8), (17, 33, 25, 49), (31, 67, 62, 134), (64, 250, 97, 511), (40, 300, 120, 900),
         (23, 29, 11, 13), (200, 300, 9, 7)]
WIDTH_CASES = [(12, 100, 20, dw) for dw in (255, 256, 257)]          # around the tile's 256 columns


def c1(x):
    return ((A + 2) * x - (A + 3)) * x * x + 1


def c2(x):
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A


def taps64(s, n):
    """(first, coef) of one axis with s source and n output samples: first[d] = floor(r) as int64 (unclamped), coef[d] the four
    float64 coefficients of source samples first - 1 .. first + 2, r = (s / n) * (d + 0.5) - 0.5."""
    d = np.arange(n, dtype=np.float64)
    r = (s / n) * (d + 0.5) - 0.5
    i = np.floor(r)
    t = r - i
    return i.astype(np.int64), np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=1)


def ref64(x, dh, dw):
    """x (..., H, W) resized to (..., dh, dw) in float64: horizontal pass, then vertical pass, tap indices clamped."""
    x = np.asarray(x, dtype=np.float64)
    sh, sw = x.shape[-2:]
    fx, cx = taps64(sw, dw)
    fy, cy = taps64(sh, dh)
    hor = sum(x[..., :, np.clip(fx - 1 + k, 0, sw - 1)] * cx[:, k] for k in range(4))
    return sum(hor[..., np.clip(fy - 1 + k, 0, sh - 1), :] * cy[:, k][:, None] for k in range(4))


def uniform(shape, seed):
    """float32 uniform [0, 1) data of the given shape."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def torch_cpu(x, dh, dw):
    """torch's own result on the CPU, float32: F.interpolate on the (..., H, W) array as a batch of planes."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape((-1, 1) + x.shape[-2:])
    y = F.interpolate(t, size=(dh, dw), mode="bicubic", align_corners=False, antialias=False)
    return y.numpy().reshape(x.shape[:-2] + (dh, dw))


@functools.lru_cache(maxsize=None)
def case(sh, sw, dh, dw):
    """(x, ref64(x), torch_cpu(x)) of one shape, computed once and shared: x float32 (sh, sw) uniform [0, 1).  Read-only."""
    x = uniform((sh, sw), 1000 * sh + sw + 7 * dh + dw)
    out = (x, ref64(x, dh, dw), torch_cpu(x, dh, dw))
    for a in out:
        a.flags.writeable = False
    return out
