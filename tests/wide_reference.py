"""Float64 restatements of SRCNN models of any widths (srcnn_set_model_shape) for the tests: torch conv2d with every layer padding
its own input (replicate or zero), generic in the channel count and in the filters n1 / n2, a row-window form, the band seams of
a model of given widths, and seeded random models whose activations keep the magnitude of the 64 / 32 generators'.

A model here is always (w1 [n1, C, 9, 9], b1 [n1], w2 [n2, n1, f2, f2], b2 [n2], w3 [C, n2, 5, 5], b3 [C]) in float32, and an
image is [C, h, w] planes."""
import numpy as np
import torch
import torch.nn.functional as F


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _conv(x, w, b, padding):
    r = (w.shape[-1] - 1) // 2
    if padding == "zero":
        return F.conv2d(x, w, b, padding=r)
    return F.conv2d(F.pad(x, (r, r, r, r), mode="replicate") if r else x, w, b)


def padded_widths(n1, n2):
    """(n1p, n2p): the widths the library pads a model to."""
    return 64 * ((n1 + 63) // 64), 32 * ((n2 + 31) // 32)


def forward(x, model, padding="replicate", dtype=torch.float64):
    """x [C, h, w] -> the values before truncation, [C, h, w], evaluated by torch on the CPU in `dtype` (float64: the reference;
    float32: the yardstick of tests/error_level.py) and returned in it."""
    w1, b1, w2, b2, w3, b3 = model
    t = _t(np.asarray(x), dtype)[None]
    t = F.relu(_conv(t, _t(w1, dtype), _t(b1, dtype), padding))
    t = F.relu(_conv(t, _t(w2, dtype), _t(b2, dtype), padding))
    return _conv(t, _t(w3, dtype), _t(b3, dtype), padding)[0].numpy()


def forward_rows(x, model, r0, r1, padding="replicate"):
    """Rows [r0, r1) of forward(x), from only the input rows they need.  Each layer pads at the TRUE image edges only: a layer's
    rows are computed on the window with the rows it needs from the layer before, cut to the image."""
    w1, b1, w2, b2, w3, b3 = model
    r2 = (w2.shape[2] - 1) // 2
    h = x.shape[1]

    def layer(t, have, want, w, b, relu):
        # t holds image rows [have[0], have[1]); return rows [want[0], want[1]) of the layer
        r = (w.shape[-1] - 1) // 2
        top, bot = want[0] - r - have[0], have[1] - (want[1] + r)    # rows of t beyond what is needed (>= 0) or missing (< 0)
        t = t[:, :, max(0, top):t.shape[2] - max(0, bot)]
        pt, pb = max(0, -top), max(0, -bot)                        # missing rows: outside the image, so padded
        t = F.pad(t, (r, r, pt, pb)) if padding == "zero" else F.pad(t, (r, r, pt, pb), mode="replicate")
        y = F.conv2d(t, _t(w), _t(b))
        return F.relu(y) if relu else y

    o = (r0, r1)
    m2 = (max(0, r0 - 2), min(h, r1 + 2))
    m1 = (max(0, m2[0] - r2), min(h, m2[1] + r2))
    m0 = (max(0, m1[0] - 4), min(h, m1[1] + 4))
    t = _t(np.asarray(x[:, m0[0]:m0[1]], np.float64))[None]
    t = layer(t, m0, m1, w1, b1, True)
    t = layer(t, m1, m2, w2, b2, True)
    return layer(t, m2, o, w3, b3, False)[0].numpy()


def band_seams(width, height, f2, n1, n2):
    """The rows where the context's row bands meet for a model of n1 / n2 filters (srcnn_spatial.cpp: two maps of
    4 (n1p + n2p) bytes per pixel within 512 MiB); for 64 / 32 the seams of spatial_reference.band_seams."""
    n1p, n2p = padded_widths(n1, n2)
    r2 = (f2 - 1) // 2
    cap = (512 << 20) // (4 * width) - n1p * (4 + 2 * r2) - n2p * 4
    band_max = max(16, cap // (n1p + n2p))
    n = (height + band_max - 1) // band_max
    band = (height + n - 1) // n
    return list(range(band, height, band))


def random_wide_model(channels, n1, f2, n2, seed):
    """A seeded model of `channels` channels and n1 / n2 filters with the magnitudes of spatial_reference.random_model and
    color_reference.random_color_model: W2's spread scaled by sqrt(64 / n1) and W3's by sqrt(32 / n2) against them, so that the
    sums over more (or fewer) channels keep their magnitude."""
    rng = np.random.default_rng(90000 + 10000 * channels + 1000 * f2 + 7 * n1 + 3 * n2 + seed)
    w1 = rng.normal(0, 0.03 / np.sqrt(channels), (n1, channels, 9, 9)).astype(np.float32)
    b1 = rng.normal(0, 1.0, n1).astype(np.float32)
    w2 = rng.normal(0, 0.08 / f2 * np.sqrt(64.0 / n1), (n2, n1, f2, f2)).astype(np.float32)
    b2 = rng.normal(0, 1.0, n2).astype(np.float32)
    w3 = rng.normal(0, 0.02 * np.sqrt(32.0 / n2), (channels, n2, 5, 5)).astype(np.float32)
    b3 = rng.normal(60, 10, channels).astype(np.float32)
    return w1, b1, w2, b2, w3, b3


def embed(model, n1, n2):
    """The model inside tensors of n1 / n2 filters: the real channels first, zero weights and zero biases after."""
    w1, b1, w2, b2, w3, b3 = model
    m1, c = w1.shape[:2]
    m2, f2 = w2.shape[0], w2.shape[2]
    W1, B1 = np.zeros((n1, c, 9, 9), np.float32), np.zeros(n1, np.float32)
    W2, B2 = np.zeros((n2, n1, f2, f2), np.float32), np.zeros(n2, np.float32)
    W3 = np.zeros((c, n2, 5, 5), np.float32)
    W1[:m1], B1[:m1], W2[:m2, :m1], B2[:m2], W3[:, :m2] = w1, b1, w2, b2, w3
    return W1, B1, W2, B2, W3, np.asarray(b3, np.float32)


def as_plain(model):
    """A 64 / 32 model in the shapes Context.set_model takes for the existing loaders: 1 channel (w1 [64,9,9], w2 [32,64] for
    f2 = 1, w3 [32,5,5], b3 a float), 3 channels as it is."""
    w1, b1, w2, b2, w3, b3 = model
    if w1.shape[1] == 3:
        return model
    return w1[:, 0], b1, (w2[:, :, 0, 0] if w2.shape[2] == 1 else w2), b2, w3[0], float(b3[0])
