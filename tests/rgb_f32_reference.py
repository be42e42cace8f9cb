"""The reference of srcnn_process_rgb_f32 (a 3-plane float image through a 1-channel model): the float32 numpy statement of the
two steps include/srcnn_amd.h adds to existing calls (the luma at the source resolution, the merge), the program the call
replaces as a float64 round trip through a full Y'CbCr matrix and its exact inverse, the colour conventions and the shapes the
CPU and GPU tests share.  Own code; nothing here calls the library under test."""
import numpy as np

from resize_f32_reference import ref64

# (sh, sw, dh, dw) of the GPU tests: the smallest shapes where the two kernels can go wrong.  Every tap clamped; an odd
# non-dyadic ratio; output column 256 crossed and several row tiles at a non-dyadic ratio; 255 / 256 / 257 columns around the
# tile's width; 15 / 16 / 17 / 33 rows around the tile's height.
SHAPES = [(1, 1, 3, 5), (5, 4, 10, 8), (17, 33, 25, 49), (64, 250, 97, 511),
          (12, 100, 20, 255), (12, 100, 20, 256), (12, 100, 20, 257),
          (9, 21, 15, 40), (9, 21, 16, 40), (9, 21, 17, 40), (9, 21, 33, 40)]
SAME_SHAPES = [(7, 5, 7, 5), (33, 300, 33, 300)]          # no resize: an image that is already up-sampled


class Convention:
    """A Y'CbCr convention for R, G, B planes holding [0, value_range]: ycc = matrix @ rgb + offset.  Its chroma rows sum to 0."""

    def __init__(self, name, matrix, offset):
        self.name = name
        self.matrix = np.asarray(matrix, dtype=np.float64)
        self.offset = np.asarray(offset, dtype=np.float64)

    def luma(self, value_range=1.0):
        """(w0, w1, w2, offset): the row the library's call takes."""
        return tuple(self.matrix[0]) + (float(self.offset[0]) * value_range,)


_KB, _KR = 0.114, 0.299
BT601_FULL = Convention("bt601-full",
                        [[_KR, 1 - _KR - _KB, _KB],
                         [-0.5 * _KR / (1 - _KB), -0.5 * (1 - _KR - _KB) / (1 - _KB), 0.5],
                         [0.5, -0.5 * (1 - _KR - _KB) / (1 - _KR), -0.5 * _KB / (1 - _KR)]],
                        [0.0, 0.5, 0.5])
# MATLAB's rgb2ycbcr
BT601_STUDIO = Convention("bt601-studio",
                          np.array([[65.481, 128.553, 24.966], [-37.797, -74.203, 112.0], [112.0, -93.786, -18.214]]) / 255.0,
                          np.array([16.0, 128.0, 128.0]) / 255.0)
# the table many SRCNN training scripts carry: 16 + (64.738 R + 129.057 G + 25.064 B) / 256 on 0..255 data
TABLE_256 = Convention("table-256",
                       np.array([[64.738, 129.057, 25.064], [-37.945, -74.494, 112.439], [112.439, -94.154, -18.285]]) / 256.0,
                       np.array([16.0, 128.0, 128.0]) / 255.0)
CONVENTIONS = [BT601_FULL, BT601_STUDIO, TABLE_256]


def gain64(luma):
    """1 / (w0 + w1 + w2) in float64 over the weights as the library holds them, float32."""
    w = np.asarray(luma[:3], dtype=np.float32).astype(np.float64)
    return 1.0 / (w[0] + w[1] + w[2])


# ---- the float32 statement of the two steps the call adds (include/srcnn_amd.h, steps 1 and 4) ------------------------------
def luma_lr_f32(x, luma):
    """Step 1: Y_lr = ((w0 x0 + w1 x1) + w2 x2) + offset on float32 planes x (3, H, W), every product and sum rounded."""
    w = np.asarray(luma, dtype=np.float32)
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[0] == 3
    y = ((w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]) + w[3]
    assert y.dtype == np.float32
    return y


def merge_f32(u, ysr, yup, g, clamp=None):
    """Step 4: out_c = U_c + (Ysr - Yup) g on float32 arrays, then the clamp: below lo -> lo, above hi -> hi, a NaN stays."""
    assert u.dtype == ysr.dtype == yup.dtype == np.float32
    out = u + ((ysr - yup) * np.float32(g))[None]
    if clamp is not None:
        lo, hi = np.float32(clamp[0]), np.float32(clamp[1])
        out = np.where(out < lo, lo, out)
        out = np.where(out > hi, hi, out)
    assert out.dtype == np.float32
    return out


# ---- the program the call replaces, in float64 -----------------------------------------------------------------------------
def classic64(x, dh, dw, conv, model64, yup=None, resize=ref64):
    """Resize the three planes, convert with the full 3 x 3 matrix, the model on Y, back through the exact inverse.  model64:
    (dh, dw) float64 -> (dh, dw) float64.  yup: a Y to hand the model instead of the converted one (the tests hand it the GPU's
    own, so that only the model's arithmetic error enters a comparison and not its sensitivity to input rounding); the chroma
    and the inverse stay those of the float64 round trip.  resize: ref64, or torch's own F.interpolate (torch_cpu)."""
    up = np.asarray(resize(x, dh, dw), dtype=np.float64)
    ycc = np.einsum("ij,jhw->ihw", conv.matrix, up) + conv.offset[:, None, None]
    ycc[0] = model64(ycc[0] if yup is None else np.asarray(yup, dtype=np.float64))
    return np.einsum("ij,jhw->ihw", np.linalg.inv(conv.matrix), ycc - conv.offset[:, None, None])


def formula64(x, dh, dw, luma, model64):
    """out_c = up(x_c) + g (Ysr - Yup) in float64, the luma row only: what the library computes in float32."""
    x = np.asarray(x, dtype=np.float64)
    w0, w1, w2, off = (float(v) for v in luma)
    yup = ref64(w0 * x[0] + w1 * x[1] + w2 * x[2] + off, dh, dw)
    return ref64(x, dh, dw) + ((model64(yup) - yup) / (w0 + w1 + w2))[None]


def standin_model(y):
    """A nonlinear, spatially mixing stand-in for an SRCNN on float64 planes (no weights needed)."""
    y = np.asarray(y, dtype=np.float64)
    mixed = 0.6 * y + 0.25 * np.roll(y, 1, axis=1) + 0.15 * np.roll(y, -1, axis=0)
    return y + 0.1 * np.sin(7.0 * mixed) + 0.05 * mixed * mixed - 0.02


def rgb(shape, seed):
    """float32 uniform [0, 1) planes (3, H, W), or (N, 3, H, W)."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)
