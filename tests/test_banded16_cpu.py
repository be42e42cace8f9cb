"""SRCNN_MODE_BANDED16 without a GPU: the mode's value, the host side of the split (scales and the W2 table, through the tuning
library's hook), a numpy model of the split arithmetic against the float64 restatements with the tolerance of SRCNN_MODE_MFMA,
and the device code of the new kernels.

The numpy model restates what the kernels compute: layer 1 in float32, every activation times 2^e1 split into
a_hi = rtz_f16(a), a_lo = f16(a - a_hi), W2 times 2^e2 split round-to-nearest (the library's own table, decoded), layer 2 as the
three products hi*hi + lo*hi + hi*lo (each exact; summed here in float64), one multiply by 2^-(e1 + e2) and the bias in float32,
layer 3 in float32.  The same model with the lo parts dropped -- plain f16 operands -- must MISS the tolerance on the 9-3-5 and
9-5-5 cases: the test can tell the split from a single f16 product.

split_model also takes one seeded defect (DEFECTS): tests/test_banded_error_level_cpu.py shows that the float32 error level of
tests/error_level.py, which the GPU tests apply to the kernels, passes the intact model and rejects every defect."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatial_listing as L
import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from color_reference import random_color_model, synth_color, torch_forward_color
from spatial_reference import as_model, pre_tolerance, random_model, torch_forward
from zero_pad_reference import torch_forward_zero

ROOT = Path(__file__).resolve().parent.parent
W, H = 130, 70


def test_mode_value_is_5_in_python_and_in_the_header():
    assert S.MODE_BANDED16 == 5
    assert "MODE_BANDED16" in S.__all__
    header = (ROOT / "include" / "srcnn_amd.h").read_text()
    assert re.search(r"\bSRCNN_MODE_BANDED16\s*=\s*5\b", header)
    modes = dict(re.findall(r"\b(SRCNN_MODE_\w+)\s*=\s*(\d+)", header))
    assert sorted(int(v) for v in modes.values()) == list(range(6))      # six distinct modes, 0 .. 5


# ---- the host side: exponents and the split W2 table ---------------------------------------------------------------------
def acc_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def l2h_channel(step, h, e):
    """K slot 8h + e of K step `step` (srcnn_kernels.h, spatial_l2h_channel)."""
    return 32 * (step >> 1) + acc_row(8 * (step & 1) + e, h)


def host_tables(model):
    """(e1, e2, w_hi, w_lo): the library's exponents, and its table decoded to two float64 arrays [32, 64, f2, f2]."""
    w1, b1, w2 = np.asarray(model[0], np.float32), np.asarray(model[1], np.float32), np.asarray(model[2], np.float32)
    channels = 3 if w1.ndim == 4 else 1
    f2 = 1 if w2.ndim == 2 else w2.shape[2]
    lib = C.CDLL(str(S.tuning_library_path()))
    fn = lib.srcnn_debug_banded16_tables
    fn.restype = C.c_int
    fp = C.POINTER(C.c_float)
    fn.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.POINTER(C.c_uint16), C.POINTER(C.c_int)]
    taps = f2 * f2
    table = np.zeros(4 * taps * 2 * 64 * 8, np.uint16)
    exps = (C.c_int * 2)()
    w1c, b1c, w2c = (np.ascontiguousarray(a.ravel()) for a in (w1, b1, w2))
    n = fn(channels, f2, w1c.ctypes.data_as(fp), b1c.ctypes.data_as(fp), w2c.ctypes.data_as(fp),
           table.ctypes.data_as(C.POINTER(C.c_uint16)), exps)
    assert n == table.nbytes
    t = table.view(np.float16).astype(np.float64).reshape(4, taps, 2, 64, 8)
    wh, wl = np.zeros((32, 64, taps)), np.zeros((32, 64, taps))
    seen = np.zeros(64, int)
    for s in range(4):
        for h in range(2):
            for e in range(8):
                ci = l2h_channel(s, h, e)
                seen[ci] += 1
                wh[:, ci, :] = t[s, :, 0, 32 * h:32 * h + 32, e].T
                wl[:, ci, :] = t[s, :, 1, 32 * h:32 * h + 32, e].T
    assert (seen == 1).all()                 # the 64 K slots are the 64 layer-1 channels, each once
    return exps[0], exps[1], wh.reshape(32, 64, f2, f2), wl.reshape(32, 64, f2, f2)


@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_w2_split_and_scales(f2, seed):
    model = random_model(f2, seed)
    e1, e2, wh, wl = host_tables(model)
    w1, b1, w2 = model[0], model[1], as_model(*model)[2]
    ws = w2.astype(np.float64) * 2.0 ** e2
    assert np.isfinite(wh).all() and np.isfinite(wl).all()
    assert 2.0 ** 14 <= np.abs(wh).max() < 2.0 ** 16
    assert (np.abs(ws - wh - wl) <= np.maximum(2.0 ** -22 * np.abs(ws), 2.0 ** -25)).all()
    # the layer-1 scale: the rigorous bound for 8-bit input lands in [2^14, 2^15)
    bound = (255.0 * np.abs(w1.astype(np.float64)).reshape(64, -1).sum(1) + np.abs(b1.astype(np.float64))).max()
    assert 2.0 ** 14 <= bound * 2.0 ** e1 < 2.0 ** 15


def test_a_model_that_cannot_be_scaled_is_refused():
    model = list(random_model(3, 0))
    model[2] = model[2].copy()
    model[2][3, 5, 1, 1] = np.inf
    with pytest.raises(AssertionError):      # the hook returns SRCNN_ERR_STATE, not the table size
        host_tables(model)


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------
def rtz_f16(a):
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(h, np.float16(0)), h)


DEFECTS = ("a_lo_one_k_step", "w_lo_one_tap", "w_lo", "a_lo", "lo_right_unit")


def split_model(x, model, padding, terms, defect=None, tables=None):
    """x [C, h, w] u8 -> the values before truncation [C, h, w] (float32 layers 1 and 3, split layer 2; terms = 1: hi * hi only).
    defect: None, or one of DEFECTS -- a seeded loss of lo parts, as a kernel could have it: a_lo dropped in K step 1 of 4 (its 16
    channels from l2h_channel), w_lo dropped on tap (0, 0), w_lo or a_lo dropped everywhere, both lo terms dropped in columns
    32 .. 63 of every 64-column tile (the right 32-column MFMA unit of spatial_l2h_kernel).  tables: host_tables(model), to
    decode the library's table once for many images."""
    assert defect is None or (defect in DEFECTS and terms == 3)
    w1, b1, w2, b2, w3, b3 = model
    w1, w3 = np.asarray(w1, np.float32), np.asarray(w3, np.float32)
    chans = x.shape[0]
    f2 = 1 if np.ndim(w2) == 2 else w2.shape[2]
    r2 = (f2 - 1) // 2
    e1, e2, wh, wl = host_tables(model) if tables is None else tables
    if defect == "w_lo":
        wl = np.zeros_like(wl)
    elif defect == "w_lo_one_tap":
        wl = wl.copy()
        wl[:, :, 0, 0] = 0

    def pad(t, r):
        return t if r == 0 else F.pad(t, (r,) * 4, mode="replicate" if padding == "replicate" else "constant")

    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    m1 = F.relu(F.conv2d(pad(t32(x)[None], 4), t32(w1.reshape(64, chans, 9, 9)), t32(b1)))[0].numpy()
    a = m1 * np.float32(2.0 ** e1)
    assert a.max() < 2.0 ** 15
    a_hi = rtz_f16(a)
    a_lo = (a - a_hi.astype(np.float32)).astype(np.float16)
    assert (a_lo >= 0).all() and np.isfinite(a_lo).all()
    if defect == "a_lo":
        a_lo = np.zeros_like(a_lo)
    elif defect == "a_lo_one_k_step":
        a_lo = a_lo.copy()
        a_lo[[l2h_channel(1, h, e) for h in range(2) for e in range(8)]] = 0
    conv = lambda act, w: F.conv2d(pad(t64(act.astype(np.float64))[None], r2), t64(w))[0].numpy()
    acc = conv(a_hi, wh)
    if terms == 3:
        # (1 or 0 per column: the intact model multiplies by 1, which changes no bit)
        keep = np.where(np.arange(x.shape[2]) % 64 >= 32, 0.0, 1.0) if defect == "lo_right_unit" else np.ones(x.shape[2])
        acc = acc + conv(a_hi, wl) * keep + conv(a_lo, wh) * keep
    m2 = np.maximum(acc.astype(np.float32).astype(np.float64) * 2.0 ** -(e1 + e2) + np.asarray(b2, np.float64)[:, None, None], 0)
    pre = F.conv2d(pad(t32(m2)[None], 2), t32(w3.reshape(chans, 32, 5, 5)), t32(np.atleast_1d(np.asarray(b3, np.float32))))
    return pre[0].numpy().astype(np.float64)


def luma_case(f2, seed, padding, terms=3):
    model = random_model(f2, seed)
    y = synth_luma(W, H, frame=seed)
    ref = torch_forward(y, model) if padding == "replicate" else torch_forward_zero(y, model)
    err = np.abs(split_model(y[None], model, padding, terms)[0] - ref).max()
    return err, pre_tolerance(ref)


def color_case(f2, seed, padding, terms=3):
    model = random_color_model(f2, seed)
    img = synth_color(W, H, frame=seed)
    ref = torch_forward_color(img, model, padding)
    pre = np.moveaxis(split_model(np.moveaxis(img, 2, 0), model, padding, terms), 0, 2)
    return np.abs(pre - ref).max(), pre_tolerance(ref)


@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_split_arithmetic_meets_the_mfma_tolerance_replicate(f2, seed):
    err, tol = luma_case(f2, seed, "replicate")
    print(f"9-{f2}-5 seed {seed}: split error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


@pytest.mark.parametrize("f2", [3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hi_parts_alone_miss_the_tolerance(f2, seed):
    """Plain f16 operands (no lo parts) are outside the contract on every 9-3-5 and 9-5-5 case: what the split buys.  (A 9-1-5
    model sums 64 products, not 576 or 1600, and its hi-only error can stay inside the tolerance: not asserted for f2 = 1.)"""
    err, tol = luma_case(f2, seed, "replicate", terms=1)
    print(f"9-{f2}-5 seed {seed}: hi-only error {err:.3g}, tolerance {tol:.3g}")
    assert err > tol


@pytest.mark.parametrize("f2", [1, 3, 5])
def test_split_arithmetic_meets_the_mfma_tolerance_zero_padding(f2):
    err, tol = luma_case(f2, 1, "zero")
    print(f"9-{f2}-5 zero padding: split error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


@pytest.mark.parametrize("padding", ["replicate", "zero"])
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_split_arithmetic_meets_the_mfma_tolerance_colour(f2, padding):
    err, tol = color_case(f2, 2, padding)
    print(f"colour 9-{f2}-5 {padding}: split error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


# ---- the device code ----------------------------------------------------------------------------------------------------------
def test_no_kernel_of_the_unit_uses_scratch_memory():
    assert len(L.kernels(L.L2H)) == 6                               # f2 = 1, 3, 5 x replicate, zero (a 64 / 32 model's forms)
    assert len(L.kernels(L.L1_BYTES)) == 8                          # 1, 3 channels x replicate, zero x f32, split output
    for name, desc, _ in L.kernels():
        assert L.private_bytes(desc) == 0, name


def test_layer2_kernel_runs_on_the_f16_mfma_only():
    found = L.kernels(L.L2H)
    assert len(found) == 6
    for name, _, body in found:
        assert "v_mfma_f32_32x32x16_f16" in body, name
        assert "v_mfma_f32_32x32x2_f32" not in body, name
