"""Float64 restatements of the SRCNN models under zero padding (srcnn_set_padding(SRCNN_PAD_ZERO)): every layer zero-pads its
own input, torch's F.conv2d(x, w, b, padding=k // 2), and an independent numpy tap loop on np.pad(mode="constant")."""
import numpy as np
import torch
import torch.nn.functional as F

from spatial_reference import as_model


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def torch_forward_zero(y, model):
    """The value before truncation, [h, w] float64, of a 9-f2-5 model with every layer zero-padding its input."""
    w1, b1, w2, b2, w3, b3 = as_model(*model)
    x = _t(y.astype(np.float64))[None, None]
    x = F.relu(F.conv2d(x, _t(w1)[:, None], _t(b1), padding=4))
    x = F.relu(F.conv2d(x, _t(w2), _t(b2), padding=(w2.shape[2] - 1) // 2))
    w3 = _t(w3)[None]
    return F.conv2d(x, w3, torch.tensor([float(b3)], dtype=torch.float64), padding=2)[0, 0].numpy()


def torch_forward_zero_rows(y, model, r0, r1):
    """Rows [r0, r1) of torch_forward_zero(y), computed from only the input rows they need.  Each layer's map is zero-padded at
    the true image edges only: inside the image the window's rows come from the rows around them, never from padding, so a
    kernel that pads where two row bands meet fails against this."""
    w1, b1, w2, b2, w3, b3 = as_model(*model)
    r2 = (w2.shape[2] - 1) // 2
    h = y.shape[0]
    # rows of every layer's output the window needs: layer 3 -> [r0, r1), layer 2 -> +-2, layer 1 -> +-(2 + r2)
    need3 = (r0, r1)
    need2 = (max(0, r0 - 2), min(h, r1 + 2))
    need1 = (max(0, need2[0] - r2), min(h, need2[1] + r2))
    need0 = (max(0, need1[0] - 4), min(h, need1[1] + 4))

    def layer(x, have, want, w, b, k):
        """x holds rows [have) of this layer's input; returns rows [want) of its output, zero-padded only off the image."""
        r = (k - 1) // 2
        top = r - (want[0] - have[0])        # rows of zeros above: only where the window reaches above row 0
        bot = r - (have[1] - want[1])
        assert top >= 0 and bot >= 0 and (top == 0 or have[0] == 0) and (bot == 0 or have[1] == h)
        xp = F.pad(x, (r, r, top, bot))      # columns: the true image edges; rows: as computed
        return F.conv2d(xp, w, b)

    x = _t(y[need0[0]:need0[1]].astype(np.float64))[None, None]
    x = F.relu(layer(x, need0, need1, _t(w1)[:, None], _t(b1), 9))
    x = F.relu(layer(x, need1, need2, _t(w2), _t(b2), 2 * r2 + 1))
    x = layer(x, need2, need3, _t(w3)[None], torch.tensor([float(b3)], dtype=torch.float64), 5)
    return x[0, 0].numpy()


def numpy_forward_zero(y, model):
    """The same model as an explicit tap loop in numpy (independent of torch's conv2d): float64, cross-correlation, each
    layer's input padded with zeros by np.pad(mode="constant")."""
    w1, b1, w2, b2, w3, b3 = as_model(*model)
    w1, w2, w3 = (np.asarray(a, np.float64) for a in (w1, w2, w3))

    def conv(x, w, b):
        k = w.shape[-1]
        r = (k - 1) // 2
        xp = np.pad(x, ((0, 0), (r, r), (r, r)), mode="constant")
        h, wd = x.shape[1:]
        out = np.zeros((w.shape[0], h, wd)) + np.asarray(b, np.float64)[:, None, None]
        for i in range(k):
            for j in range(k):
                out += np.einsum("oc,chw->ohw", w[:, :, i, j], xp[:, i:i + h, j:j + wd])
        return out

    x = np.maximum(conv(y.astype(np.float64)[None], w1.reshape(64, 1, 9, 9), b1), 0)
    x = np.maximum(conv(x, w2, b2), 0)
    return conv(x, w3.reshape(1, 32, 5, 5), [b3])[0]
