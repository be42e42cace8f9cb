"""What the command-line tool (tools/srcnn_cli.cpp) must write, stated without the product: bitwise expectations for the shipped
9-1-5 model (oracle.process_bgr), float64 compositions for the models that have no bitwise CPU model (9-3-5, 9-5-5, zero
padding, colour), and models whose output is a picture, so that a blob sliced at a wrong offset cannot pass."""
import numpy as np

import oracle
from color_reference import color_blob, torch_forward_color
from spatial_reference import model_blob, pre_tolerance, u8_of
from spatial_reference import torch_forward
from zero_pad_reference import torch_forward_zero

AMBIGUOUS_CAP = 0.03        # share of pixels whose float64 value lies within the tolerance of an integer
MIN_LEVELS = 64             # distinct output bytes of the reference: a picture, not a flat grey


def expected_bgr_915(bgr, scale, blob, mode):
    """The tool's bytes with the shipped model: --refbytes -> the reference arithmetic, default -> the FMA-order model."""
    if mode == "refbytes":
        return oracle.process_bgr(bgr, scale, blob)
    assert mode == "default"
    return oracle.process_bgr(bgr, scale, blob, y_path=oracle.gpuorder_forward_y)


def centre_tap_model(blob, f2, seed):
    """The shipped 9-1-5 tables as a 9-f2-5 model: W2 at the centre tap of an f2 x f2 kernel, the other taps seeded
    N(0, 0.05 max|W2|).  Unlike spatial_reference.random_model its output on a synthetic picture spans > 100 grey levels."""
    w1, b1, w2, b2, w3, b3 = oracle.split_weights(blob)
    if f2 == 1:
        return w1, b1, w2, b2, w3, b3
    rng = np.random.default_rng(500 + 10 * f2 + seed)
    k = rng.normal(0, 0.05 * float(np.abs(w2).max()), (32, 64, f2, f2)).astype(np.float32)
    k[:, :, f2 // 2, f2 // 2] = w2
    return w1, b1, k, b2, w3, b3


def centre_tap_color_model(blob, f2, seed):
    """A colour model built from the shipped tables: layer 1 reads the BT.601 luma of the three channels (plus seeded noise
    that tells the channels apart), layer 2 as centre_tap_model, layer 3 the shipped W3 for every output channel with seeded
    noise and a different bias each -- three different pictures, so a shifted or permuted table shows."""
    w1, b1, w2, b2, w3, b3 = centre_tap_model(blob, f2, seed)
    rng = np.random.default_rng(900 + 10 * f2 + seed)
    mix = np.array([0.114, 0.587, 0.299], np.float32)                       # B, G, R
    cw1 = w1[:, None] * mix[None, :, None, None] + rng.normal(0, 0.02 * float(np.abs(w1).max()), (64, 3, 9, 9))
    cw2 = w2.reshape(32, 64, f2, f2)
    cw3 = w3[None] + rng.normal(0, 0.05 * float(np.abs(w3).max()), (3, 32, 5, 5))
    cb3 = b3 + np.array([-12.0, 0.0, 9.0])
    return cw1.astype(np.float32), b1, cw2, b2, cw3.astype(np.float32), cb3.astype(np.float32)


def luma_reference(bgr, scale, model, padding):
    """float64 composition for a 1-channel model: colour conversion and three bicubic resizes as the oracle does them, then
    the model on the resized Y -> (ref_pre [oh, ow] float64, cr, cb)."""
    h, w, _ = bgr.shape
    ow, oh = oracle.scaled_size(w, h, scale)
    y, cr, cb = (oracle.resize_cubic(p, ow, oh) for p in oracle.bgr2ycrcb(bgr))
    fwd = torch_forward_zero if padding == "zero" else torch_forward
    return fwd(y, model), cr, cb


def color_reference(bgr, scale, model, padding):
    """float64 composition for a colour model: the three channels resized as they are, no colour conversion -> [oh, ow, 3]."""
    h, w, _ = bgr.shape
    ow, oh = oracle.scaled_size(w, h, scale)
    up = np.stack([oracle.resize_cubic(np.ascontiguousarray(bgr[:, :, c]), ow, oh) for c in range(3)], axis=2)
    return torch_forward_color(up, model, padding)


def ambiguous(ref_pre):
    """(mask of the values within the project's tolerance of an integer, that tolerance)."""
    tol = pre_tolerance(ref_pre)
    return np.abs(ref_pre - np.rint(ref_pre)) <= tol, tol


def assert_is_a_picture(ref_pre):
    """The two conditions on a case's inputs, from the reference alone -> the ambiguous share."""
    amb, _ = ambiguous(ref_pre)
    levels = len(np.unique(u8_of(ref_pre)))
    assert levels >= MIN_LEVELS, f"the reference spans {levels} output bytes only"
    assert amb.mean() <= AMBIGUOUS_CAP, f"ambiguous share {amb.mean():.4f} above {AMBIGUOUS_CAP}"
    return float(amb.mean())


def assert_bgr_of_luma(out, ref_pre, cr, cb):
    """out [oh, ow, 3] against the float64 luma: where ref_pre is not ambiguous the three bytes are the conversion of
    trunc-and-clamp(ref_pre); where it is, of the byte just below or just above that integer.  Returns the ambiguous share."""
    assert out.shape == ref_pre.shape + (3,) and out.dtype == np.uint8
    amb, _ = ambiguous(ref_pre)
    n = np.rint(ref_pre)
    y = u8_of(ref_pre)
    lo = oracle.ycrcb2bgr(np.where(amb, u8_of(n - 0.5), y), cr, cb)
    hi = oracle.ycrcb2bgr(np.where(amb, u8_of(n + 0.5), y), cr, cb)
    is_lo, is_hi = (out == lo).all(axis=2), (out == hi).all(axis=2)
    share = float(amb.mean())
    bad = ~(is_lo | is_hi)
    assert not (bad & ~amb).any(), f"{(bad & ~amb).sum()} unambiguous pixels differ (ambiguous share {share:.4f})"
    assert not bad.any(), f"{bad.sum()} ambiguous pixels match neither neighbouring byte (ambiguous share {share:.4f})"
    return share


__all__ = ["AMBIGUOUS_CAP", "MIN_LEVELS", "expected_bgr_915", "centre_tap_model", "centre_tap_color_model", "luma_reference",
           "color_reference", "ambiguous", "assert_is_a_picture", "assert_bgr_of_luma", "model_blob", "color_blob"]
