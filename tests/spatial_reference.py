"""Float64 restatements of the 9-f2-5 SRCNN models (srcnn_set_model) for the tests: torch conv2d with every layer
replicate-padding its own input, an independent numpy loop, and seeded random models that do not saturate on synth_luma."""
import numpy as np
import torch
import torch.nn.functional as F


def as_model(w1, b1, w2, b2, w3, b3):
    """(w1, b1, w2[32,64,f2,f2], b2, w3, b3) with a 9-1-5 w2 [32,64] lifted to [32,64,1,1]."""
    w2 = np.asarray(w2)
    return w1, b1, (w2.reshape(32, 64, 1, 1) if w2.ndim == 2 else w2), b2, w3, b3


def torch_layers12(y, model):
    """The 32-channel layer-2 map [32, h, w] in float64."""
    w1, b1, w2, b2, _, _ = as_model(*model)
    r2 = (w2.shape[2] - 1) // 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    x = t(y.astype(np.float64))[None, None]
    x = F.relu(F.conv2d(F.pad(x, (4, 4, 4, 4), mode="replicate"), t(w1)[:, None], t(b1)))
    if r2:
        x = F.pad(x, (r2, r2, r2, r2), mode="replicate")
    return F.relu(F.conv2d(x, t(w2), t(b2)))[0]


def torch_layer3(map32, model):
    """Layer 3 of a float64 [32, h, w] map (tensor or array): the value before truncation, [h, w] float64."""
    _, _, _, _, w3, b3 = model
    x = torch.as_tensor(np.asarray(map32, dtype=np.float64))[None]
    w = torch.from_numpy(np.ascontiguousarray(w3, dtype=np.float64))[None]
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode="replicate"), w, torch.tensor([float(b3)], dtype=torch.float64))[0, 0].numpy()


def torch_forward(y, model):
    return torch_layer3(torch_layers12(y, model), model)


def torch_forward_rows(y, model, r0, r1):
    """Rows [r0, r1) of torch_forward(y), computed from only the input rows they need (true image edges replicated)."""
    _, _, w2, _, _, _ = as_model(*model)
    reach = 4 + (w2.shape[2] - 1) // 2 + 2
    a, b = max(0, r0 - reach), min(y.shape[0], r1 + reach)
    return torch_forward(y[a:b], model)[r0 - a:r1 - a]


def numpy_forward(y, model):
    """The same model as an explicit tap loop in numpy (independent of torch's conv2d): float64, cross-correlation."""
    w1, b1, w2, b2, w3, b3 = as_model(*model)
    w1, w2, w3 = (np.asarray(a, np.float64) for a in (w1, w2, w3))

    def conv(x, w, b):                       # x [cin, h, w], w [cout, cin, k, k]: replicate-pad x, correlate
        k = w.shape[-1]
        r = (k - 1) // 2
        xp = np.pad(x, ((0, 0), (r, r), (r, r)), mode="edge")
        h, wd = x.shape[1:]
        out = np.zeros((w.shape[0], h, wd)) + np.asarray(b, np.float64)[:, None, None]
        for i in range(k):
            for j in range(k):
                out += np.einsum("oc,chw->ohw", w[:, :, i, j], xp[:, i:i + h, j:j + wd])
        return out

    x = np.maximum(conv(y.astype(np.float64)[None], w1.reshape(64, 1, 9, 9), b1), 0)
    x = np.maximum(conv(x, w2, b2), 0)
    return conv(x, w3.reshape(1, 32, 5, 5), [b3])[0]


def random_model(f2, seed):
    """A seeded 9-f2-5 model with the magnitudes of test_random_weights_all_modes, W2's spread scaled down by f2."""
    rng = np.random.default_rng(1000 * f2 + seed)
    w1 = rng.normal(0, 0.03, (64, 9, 9)).astype(np.float32)
    b1 = rng.normal(0, 1.0, 64).astype(np.float32)
    w2 = rng.normal(0, 0.08 / f2, (32, 64, f2, f2) if f2 > 1 else (32, 64)).astype(np.float32)
    b2 = rng.normal(0, 1.0, 32).astype(np.float32)
    w3 = rng.normal(0, 0.02, (32, 5, 5)).astype(np.float32)
    b3 = float(np.float32(rng.normal(60, 10)))
    return w1, b1, w2, b2, w3, b3


def model_blob(model):
    w1, b1, w2, b2, w3, b3 = model
    return np.concatenate([np.ravel(b1), np.ravel(w1), np.ravel(b2), np.ravel(w2), [b3], np.ravel(w3)]).astype(np.float32)


def band_seams(width, height, f2):
    """The rows where the context's row bands meet (srcnn_spatial.cpp: two maps of 384 B per pixel within 512 MiB), for a model
    of any channel count."""
    r2 = (f2 - 1) // 2
    cap = (512 << 20) // (4 * width) - 64 * (4 + 2 * r2) - 32 * 4
    band_max = max(16, cap // 96)
    n = (height + band_max - 1) // band_max
    band = (height + n - 1) // n
    return list(range(band, height, band))


def pre_tolerance(ref):
    return 5e-3 * max(1.0, float(np.abs(ref).max()) / 255.0)


def u8_of(pre):
    return np.clip(np.trunc(pre), 0, 255).astype(np.uint8)


def assert_u8_consistent(out, ref_pre, tol):
    """out within 1 LSB of trunc(ref_pre), and differing only where ref_pre lies within tol of an integer."""
    d = np.abs(out.astype(int) - u8_of(ref_pre).astype(int))
    assert d.max() <= 1, f"u8 differs by {d.max()} LSB"
    if d.any():
        assert np.abs(ref_pre - np.rint(ref_pre))[d != 0].max() <= tol

