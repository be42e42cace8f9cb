"""Float64 restatements of the colour SRCNN models (srcnn_set_model_color) for the tests: torch conv2d with every layer padding
its own input (replicate or zero), an independent numpy tap loop, a row-window form, and seeded random colour models with the
magnitudes of spatial_reference.random_model."""
import numpy as np
import torch
import torch.nn.functional as F


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _conv(x, w, b, padding):
    r = (w.shape[-1] - 1) // 2
    if padding == "zero":
        return F.conv2d(x, w, b, padding=r)
    return F.conv2d(F.pad(x, (r, r, r, r), mode="replicate") if r else x, w, b)


def as_color_model(w1, b1, w2, b2, w3, b3):
    """(w1[64,3,9,9], b1, w2[32,64,f2,f2], b2, w3[3,32,5,5], b3[3]) with a 1x1 w2 [32,64] lifted to [32,64,1,1]."""
    w2 = np.asarray(w2)
    return w1, b1, (w2.reshape(32, 64, 1, 1) if w2.ndim == 2 else w2), b2, w3, np.asarray(b3)


def torch_forward_color(img, model, padding="replicate"):
    """img [h, w, 3] (interleaved channels) -> the values before truncation, [h, w, 3] float64."""
    w1, b1, w2, b2, w3, b3 = as_color_model(*model)
    x = _t(np.moveaxis(np.asarray(img, np.float64), 2, 0))[None]
    x = F.relu(_conv(x, _t(w1), _t(b1), padding))
    x = F.relu(_conv(x, _t(w2), _t(b2), padding))
    x = _conv(x, _t(w3), _t(b3), padding)
    return np.moveaxis(x[0].numpy(), 0, 2)


def torch_forward_color_rows(img, model, r0, r1, padding="replicate"):
    """Rows [r0, r1) of torch_forward_color(img), from only the input rows they need.  Each layer pads at the TRUE image edges
    only: a layer's rows are computed on the window with the rows it needs from the layer before, cut to the image."""
    w1, b1, w2, b2, w3, b3 = as_color_model(*model)
    r2 = (w2.shape[2] - 1) // 2
    h = img.shape[0]

    def layer(x, have, want, w, b, relu):
        # x holds image rows [have[0], have[1]); return rows [want[0], want[1]) of the layer
        k = w.shape[-1]
        r = (k - 1) // 2
        top, bot = want[0] - r - have[0], have[1] - (want[1] + r)    # rows of x beyond what is needed (>= 0) or missing (< 0)
        x = x[:, :, max(0, top):x.shape[2] - max(0, bot)]
        pt, pb = max(0, -top), max(0, -bot)                        # missing rows: outside the image, so padded
        if padding == "zero":
            x = F.pad(x, (r, r, pt, pb))
        else:
            x = F.pad(x, (r, r, pt, pb), mode="replicate")
        y = F.conv2d(x, _t(w), _t(b))
        return F.relu(y) if relu else y

    o = (r0, r1)
    m2 = (max(0, r0 - 2), min(h, r1 + 2))
    m1 = (max(0, m2[0] - r2), min(h, m2[1] + r2))
    m0 = (max(0, m1[0] - 4), min(h, m1[1] + 4))
    x = _t(np.moveaxis(np.asarray(img[m0[0]:m0[1]], np.float64), 2, 0))[None]
    x = layer(x, m0, m1, w1, b1, True)
    x = layer(x, m1, m2, w2, b2, True)
    x = layer(x, m2, o, w3, b3, False)
    return np.moveaxis(x[0].numpy(), 0, 2)


def numpy_forward_color(img, model, padding="replicate"):
    """The same model as an explicit tap loop in numpy (independent of torch's conv2d): float64, cross-correlation."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, np.float64) for a in as_color_model(*model))

    def conv(x, w, b):                       # x [cin, h, w], w [cout, cin, k, k]
        r = (w.shape[-1] - 1) // 2
        xp = np.pad(x, ((0, 0), (r, r), (r, r)), mode="constant" if padding == "zero" else "edge")
        h, wd = x.shape[1:]
        out = np.zeros((w.shape[0], h, wd)) + b[:, None, None]
        for i in range(w.shape[-1]):
            for j in range(w.shape[-1]):
                out += np.einsum("oc,chw->ohw", w[:, :, i, j], xp[:, i:i + h, j:j + wd])
        return out

    x = np.moveaxis(np.asarray(img, np.float64), 2, 0)
    x = np.maximum(conv(x, w1, b1), 0)
    x = np.maximum(conv(x, w2, b2), 0)
    return np.moveaxis(conv(x, w3, b3), 0, 2)


def random_color_model(f2, seed):
    """A seeded colour 9-f2-5 model: random_model's magnitudes, W1's spread divided by sqrt(3) for its three input channels."""
    rng = np.random.default_rng(7000 + 1000 * f2 + seed)
    w1 = rng.normal(0, 0.03 / np.sqrt(3), (64, 3, 9, 9)).astype(np.float32)
    b1 = rng.normal(0, 1.0, 64).astype(np.float32)
    w2 = rng.normal(0, 0.08 / f2, (32, 64, f2, f2)).astype(np.float32)
    b2 = rng.normal(0, 1.0, 32).astype(np.float32)
    w3 = rng.normal(0, 0.02, (3, 32, 5, 5)).astype(np.float32)
    b3 = rng.normal(60, 10, 3).astype(np.float32)
    return w1, b1, w2, b2, w3, b3


def color_blob(model):
    """b1 | W1 | b2 | W2 | b3[3] | W3 as float32 (srcnn_set_model_color's blob form)."""
    w1, b1, w2, b2, w3, b3 = model
    return np.concatenate([np.ravel(b1), np.ravel(w1), np.ravel(b2), np.ravel(w2), np.ravel(b3), np.ravel(w3)]).astype(np.float32)


def synth_color(w, h, frame=0):
    """A deterministic interleaved 3-channel test image built from synth_luma: three differently shifted planes."""
    from srcnn_cpp_amd.synth import synth_luma
    y = synth_luma(w, h, frame=frame)
    return np.ascontiguousarray(np.stack([y, np.roll(y[::-1], 3, axis=1), np.roll(y[:, ::-1], 5, axis=0)], axis=2))
