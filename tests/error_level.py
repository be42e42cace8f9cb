"""The float32 error level: the yardstick the banded path (srcnn_spatial.cpp, srcnn_spatial_kernels.hip) is held to.

The banded kernels have no bitwise CPU model (the summation order inside an MFMA is not documented), and the project's
tolerance pre_tolerance(ref) = 5e-3 max(1, max |ref| / 255) is several hundred times the error of a correct float32
evaluation: a lost cross term of the split-f16 layer 2, a stray f16 conversion or a reduced-precision MFMA hides under it.
Here the bound comes from the reference alone:

  Y = the deviation of a plain float32 evaluation (torch, CPU) of the same model on the same images from the float64 one,
      its maximum Y.max and its root mean square Y.rms POOLED over all images of a case -- on a 1 x 1 or 3 x 3 plane the
      realised float32 error can be anything down to 0, while the error level belongs to the model and the statistics of the
      data, not to the shape;
  a result passes when, on every plane, max |out - ref64| <= MAX_FACTOR Y.max and, pooled over the planes like the yardstick,
      rms(out - ref64) <= RMS_FACTOR Y.rms.

Any order of float32 summation has the same first-order error bound, so a correct kernel sits near 1 on this scale whatever
its order (the GPU errors recorded in DESIGN.md are 1 to 2); the smallest seeded defect of tests/test_banded_error_level_cpu.py
sits at 15 or more.  MAX_FACTOR = 4 leaves a factor 2 over what was recorded and nearly 4 under the smallest defect.  The
factors may only be raised (to at most 8, half the smallest defect) for a reason found in a kernel's arithmetic and written
into DESIGN.md; nothing here is ever measured on a GPU mode.

SHAPES are the smallest planes that put an edge of each banded kernel's tile at, one before and one after the image edge,
derived from the tile constants in the kernel unit's source text."""
import functools
import re
from collections import namedtuple
from pathlib import Path

import numpy as np
import torch

import wide_reference
from color_reference import random_color_model, synth_color
from spatial_reference import as_model, random_model
from srcnn_cpp_amd.synth import synth_luma

MAX_FACTOR, RMS_FACTOR = 4.0, 3.0
KERNEL_UNIT = Path(__file__).resolve().parent.parent / "srcnn_cpp_amd" / "csrc" / "srcnn_spatial_kernels.hip"
TILE_NAMES = ("SL1_COLS", "SL1_ROWS", "SL2_COLS", "SL2_ROWS", "SL3_COLS", "SL3_SEG", "SL3_XCDS")


def forward(x, model, padding, dtype):
    """x [C, h, w] -> the values before truncation [C, h, w] of a model of any channel count and widths, by torch on the CPU in
    `dtype`: wide_reference.forward (torch.float64: the reference; torch.float32: the yardstick)."""
    return wide_reference.forward(x, model, padding, dtype)


Yardstick = namedtuple("Yardstick", "max rms refs")


def yardstick(model, padding, images):
    """Yardstick(max, rms, refs): the largest and the root-mean-square deviation of the float32 evaluation from the float64 one,
    pooled over all `images` ([C, h, w] each), and the float64 references of the images, in order."""
    refs = [forward(x, model, padding, torch.float64) for x in images]
    devs = [forward(x, model, padding, torch.float32).astype(np.float64) - r for x, r in zip(images, refs)]
    pooled = np.concatenate([d.ravel() for d in devs])
    return Yardstick(float(np.abs(pooled).max()), float(np.sqrt(np.mean(pooled ** 2))), refs)


def ratios(outs, y):
    """(largest max |out - ref| / Y.max over the planes, pooled rms / Y.rms) of results `outs` ([C, h, w] each, in the order of
    the yardstick's images)."""
    assert len(outs) == len(y.refs)
    devs = []
    for out, ref in zip(outs, y.refs):
        out = np.asarray(out)
        assert out.shape == ref.shape and np.isfinite(out).all()
        devs.append(out.astype(np.float64) - ref)
    pooled = np.concatenate([d.ravel() for d in devs])
    return max(float(np.abs(d).max()) for d in devs) / y.max, float(np.sqrt(np.mean(pooled ** 2))) / y.rms


def check(outs, y, what):
    """The assertion of the error level, on the CPU models and on the GPU alike; prints the case's line and returns the ratios."""
    r_max, r_rms = ratios(outs, y)
    print(f"{what}: max / Y_max = {r_max:.2f}, rms / Y_rms = {r_rms:.2f}   (Y_max {y.max:.3g}, Y_rms {y.rms:.3g})")
    assert r_max <= MAX_FACTOR, f"{what}: max error {r_max:.2f} x the float32 level {y.max:.3g} (bound {MAX_FACTOR})"
    assert r_rms <= RMS_FACTOR, f"{what}: rms error {r_rms:.2f} x the float32 level {y.rms:.3g} (bound {RMS_FACTOR})"
    return r_max, r_rms


# ---- shapes -------------------------------------------------------------------------------------------------------------------
def tile_constants(text=None):
    """{name: value} of TILE_NAMES, read from the `constexpr int` lines of the kernel unit's source text."""
    text = KERNEL_UNIT.read_text() if text is None else text
    found = {}
    for line in re.findall(r"^constexpr int ([^;]*);", text, flags=re.M):
        for name, value in re.findall(r"\b(\w+) = (\d+)\b", line):
            if name in TILE_NAMES:
                assert name not in found, name
                found[name] = int(value)
    assert sorted(found) == sorted(TILE_NAMES), found
    return found


def l3_tiles(w, h, k):
    """The tiles of layer 3 on a w x h plane of one band: 124-column strips (4 of the 128 map columns are halo) x row segments."""
    out = k["SL3_COLS"] - 4
    return ((w + out - 1) // out) * ((h + k["SL3_SEG"] - 1) // k["SL3_SEG"])


def shapes(k):
    """(w, h) planes for tile constants k: 1 x 1, widths 2 and 3, every column bound (layer 2's 64, layer 3's 124 output
    columns, layer 1's 128) and every row bound (8, 16, 16) at - 1, 0, + 1, a second tile bound + 1 in both directions (with a
    layer-3 tile count that is no multiple of the XCD count), and the smallest two-strip plane whose tile count is one."""
    c2, c3, c1 = k["SL2_COLS"], k["SL3_COLS"] - 4, k["SL1_COLS"]
    r1, r2, r3, xcds = k["SL1_ROWS"], k["SL2_ROWS"], k["SL3_SEG"], k["SL3_XCDS"]
    out = [(1, 1), (2, 5), (3, 3),
           (c2 - 1, r1 - 1), (c2, r1), (c2 + 1, r1 + 1),
           (c3 - 1, r2 - 1), (c3, r2 - 1), (c3 + 1, r2),
           (c1 - 1, r2 + 1), (c1, r2), (c1 + 1, r2 + 1),
           (2 * c3 + 1, 2 * r3 + 1),                           # 3 x 3 layer-3 tiles: blocks return early, two tiles on one XCD
           (c3 + 1, r3 * (xcds // 2 - 1) + 1)]                 # 2 x xcds / 2 tiles: every block of the grid has a tile
    for rows in sorted({r + d for r in (r1, r2, r3) for d in (-1, 0, 1)} - {h for _, h in out}):
        out.append((5, rows))                                  # (a row bound the list above does not reach: none while r2 = r3)
    return out


def short_shapes(k):
    """1 x 1 and the first tile bound of each layer, for the wide models."""
    return [(1, 1), (k["SL2_COLS"], k["SL1_ROWS"]), (k["SL3_COLS"] - 4, k["SL2_ROWS"] - 1), (k["SL1_COLS"], k["SL2_ROWS"])]


SHAPES = shapes(tile_constants())
SHORT_SHAPES = short_shapes(tile_constants())


# ---- cases: models and images -------------------------------------------------------------------------------------------------
def narrow_model(channels, f2, seed):
    """(the model as Context.set_model takes it, the same model in wide_reference's generic form) of 64 / 32 filters: the
    generators of the banded tests, random_model and random_color_model."""
    if channels == 3:
        plain = random_color_model(f2, seed)
        return plain, plain
    plain = random_model(f2, seed)
    w1, b1, w2, b2, w3, b3 = as_model(*plain)
    return plain, (w1[:, None], b1, w2, b2, w3[None], np.array([b3], np.float32))


def unit_model(model):
    """The model for [0, 1] data: W1 times 255 (rounded to float32: this IS the model, for the library and the reference alike),
    so that its activations are those of the 8-bit model on 255 x."""
    return (np.asarray(model[0], np.float32) * np.float32(255.0),) + tuple(model[1:])


def byte_images(channels, seed, shape_list=None):
    """[C, h, w] uint8 planes of every shape: synth_luma, or the three planes of synth_color."""
    out = []
    for w, h in SHAPES if shape_list is None else shape_list:
        x = synth_color(w, h, frame=seed) if channels == 3 else synth_luma(w, h, frame=seed)[:, :, None]
        out.append(np.ascontiguousarray(np.moveaxis(x, 2, 0)))
    return out


def float_images(images, unit):
    """The byte images as float32: integer-valued, or over 255 (in [0, 1])."""
    return [x.astype(np.float32) / np.float32(255.0) if unit else x.astype(np.float32) for x in images]


@functools.lru_cache(maxsize=None)
def narrow_case(channels, f2, padding, unit, seed=0, short=False):
    """(plain model, generic model, images, yardstick) of one 64 / 32 case; unit: [0, 1] float data and unit_model.  The byte
    forms and the integer-valued float form share the case unit = False (the float64 reference of x and of float32(x) is one)."""
    plain, model = narrow_model(channels, f2, seed)
    images = byte_images(channels, seed, SHORT_SHAPES if short else None)
    if unit:
        plain, model, images = unit_model(plain), unit_model(model), float_images(images, True)
    return plain, model, images, yardstick(model, padding, images)


@functools.lru_cache(maxsize=None)
def wide_case(channels, n1, f2, n2, padding, unit, seed=0):
    """(model, images, yardstick) of one wide case (wide_reference.random_wide_model) on SHORT_SHAPES."""
    model = wide_reference.random_wide_model(channels, n1, f2, n2, seed)
    images = byte_images(channels, seed, SHORT_SHAPES)
    if unit:
        model, images = unit_model(model), float_images(images, True)
    return model, images, yardstick(model, padding, images)
