"""Layer 2 of a wide model in split f16 (srcnn_set_wide_split16) without a GPU: the ABI, the host side of
the split for padded widths n1p / n2p (scales and the W2 table, through the tuning library's hook), a numpy model of the split
arithmetic against the float64 restatement, and the device code of the wide forms of spatial_l2h_kernel.

The numpy model is tests/test_banded16_cpu.py's split_model for any widths: layer 1 in float32, every activation times 2^e1
split into a_hi = rtz_f16(a), a_lo = f16(a - a_hi), W2 times 2^e2 split round-to-nearest (the library's own table, decoded),
layer 2 as the three products hi*hi + lo*hi + hi*lo (each exact; summed here in float64), one multiply by 2^-(e1 + e2) and the
bias in float32, layer 3 in float32.  The tolerance is that of tests/test_gpu_wide.py: pre_tolerance(ref) * max(n1p / 64,
n2p / 32)."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd.synth import synth_luma
import spatial_listing as L
from color_reference import synth_color
from spatial_reference import as_model, pre_tolerance, random_model
from wide_reference import embed, forward, padded_widths, random_wide_model

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["srcnn_set_wide_split16", "srcnn_get_wide_split16"]
UNIT = "srcnn_wide16_kernels.hip"
W, H = 130, 70
WIDTHS = [(128, 64), (128, 32), (64, 64), (100, 40)]


@pytest.fixture(scope="module")
def lib():
    B.build()
    return S.load_library()


# ---- 1: the ABI -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_option(lib):
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in srcnn_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in S.ABI_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    assert set(NEW_SYMBOLS) <= {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert lib.srcnn_abi_version() == 1                      # a plain addition: no version bump
    modes = dict(re.findall(r"\b(SRCNN_MODE_\w+)\s*=\s*(\d+)", text))
    assert sorted(int(v) for v in modes.values()) == list(range(6))      # an option, not a mode: still the six modes 0 .. 5
    assert callable(S.Context.set_wide_split16) and callable(S.Context.wide_split16)


def test_null_context_and_the_unit_is_gone_from_the_build_and_from_disk(lib):
    assert lib.srcnn_set_wide_split16(None, 1) == S.ERR_INVALID
    assert lib.srcnn_get_wide_split16(None) == S.ERR_INVALID
    assert UNIT not in [u[0] for u in B.UNITS] and not (B.CSRC / UNIT).exists()


# ---- 2: the host side: exponents and the split W2 table -------------------------------------------------------------------
def acc_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def l2h_channel(step, h, e):
    """Layer-1 channel of K slot 8h + e of K step `step` of n1p / 16 (srcnn_kernels.h: spatial_l2h_channel inside a group of 64)."""
    return 64 * (step >> 2) + 32 * ((step & 3) >> 1) + acc_row(8 * (step & 1) + e, h)


def padded(model):
    """The model in tensors of its padded widths, and (channels, n1p, n2p, f2)."""
    w1, w2 = model[0], model[2]
    n1p, n2p = padded_widths(w1.shape[0], w2.shape[0])
    return embed(model, n1p, n2p), (w1.shape[1], n1p, n2p, w2.shape[2])


def hook():
    lib = C.CDLL(str(S.tuning_library_path()))
    fn = lib.srcnn_debug_wide16_tables
    fn.restype = C.c_int
    fp = C.POINTER(C.c_float)
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_float, C.POINTER(C.c_uint16), C.POINTER(C.c_int)]
    return lib, fn, fp


def raw_tables(model, rng_max=255.0):
    """(return code, table uint16, (e1, e2)) of the hook for the padded model."""
    pm, (channels, n1p, n2p, f2) = padded(model)
    _, fn, fp = hook()
    table = np.zeros((n2p // 32) * (n1p // 16) * f2 * f2 * 2 * 64 * 8, np.uint16)
    exps = (C.c_int * 2)()
    w1c, b1c, w2c = (np.ascontiguousarray(np.asarray(a, np.float32).ravel()) for a in pm[:3])
    rc = fn(channels, n1p, n2p, f2, w1c.ctypes.data_as(fp), b1c.ctypes.data_as(fp), w2c.ctypes.data_as(fp), rng_max,
            table.ctypes.data_as(C.POINTER(C.c_uint16)), exps)
    return rc, table, (exps[0], exps[1])


@functools.lru_cache(maxsize=None)
def _tables_cached(key):
    model = MODELS[key]
    pm, (channels, n1p, n2p, f2) = padded(model)
    rc, table, (e1, e2) = raw_tables(model)
    assert rc == table.nbytes, rc
    taps = f2 * f2
    t = table.view(np.float16).astype(np.float64).reshape(n2p // 32, n1p // 16, taps, 2, 64, 8)
    wh, wl = np.zeros((n2p, n1p, taps)), np.zeros((n2p, n1p, taps))
    seen = np.zeros((n2p, n1p), int)
    for g in range(n2p // 32):
        for s in range(n1p // 16):
            for h in range(2):
                for e in range(8):
                    ci = l2h_channel(s, h, e)
                    seen[32 * g:32 * g + 32, ci] += 1
                    wh[32 * g:32 * g + 32, ci, :] = t[g, s, :, 0, 32 * h:32 * h + 32, e].T
                    wl[32 * g:32 * g + 32, ci, :] = t[g, s, :, 1, 32 * h:32 * h + 32, e].T
    assert (seen == 1).all()             # every (output channel, input channel) pair of the padded model, each once
    return e1, e2, wh.reshape(n2p, n1p, f2, f2), wl.reshape(n2p, n1p, f2, f2)


MODELS = {}


def host_tables(model, key):
    """(e1, e2, w_hi, w_lo): the library's exponents, and its table decoded to two float64 arrays [n2p, n1p, f2, f2]."""
    MODELS[key] = model
    return _tables_cached(key)


@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("n1,n2", WIDTHS)
@pytest.mark.parametrize("channels", [1, 3])
def test_w2_split_and_scales(channels, n1, n2, f2):
    model = random_wide_model(channels, n1, f2, n2, 21)
    e1, e2, wh, wl = host_tables(model, ("t", channels, n1, n2, f2))
    pm, (_, n1p, n2p, _) = padded(model)
    ws = pm[2].astype(np.float64) * 2.0 ** e2
    assert np.isfinite(wh).all() and np.isfinite(wl).all()
    assert (np.abs(ws - wh - wl) <= np.maximum(2.0 ** -22 * np.abs(ws), 2.0 ** -25)).all()
    assert 2.0 ** 14 <= np.abs(ws).max() < 2.0 ** 15
    # the padding is zeros in both halves
    assert not wh[n2:].any() and not wl[n2:].any() and not wh[:, n1:].any() and not wl[:, n1:].any()
    # the layer-1 scale: the rigorous bound for 8-bit input over all n1p channels lands in [2^14, 2^15)
    bound = (255.0 * np.abs(pm[0].astype(np.float64)).reshape(n1p, -1).sum(1) + np.abs(pm[1].astype(np.float64))).max()
    assert 2.0 ** 14 <= bound * 2.0 ** e1 < 2.0 ** 15
    # ... and follows the range of a float call; the table and e2 do not
    rc, table1, (e1u, e2u) = raw_tables(model, 1.0)
    bound = (np.abs(pm[0].astype(np.float64)).reshape(n1p, -1).sum(1) + np.abs(pm[1].astype(np.float64))).max()
    assert rc == table1.nbytes and e2u == e2 and 2.0 ** 14 <= bound * 2.0 ** e1u < 2.0 ** 15
    assert np.array_equal(table1, raw_tables(model)[1])


@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_64_32_table_is_the_table_of_banded16(channels, f2):
    """One packer: for n1p = 64 and n2p = 32 the bytes and the exponents of srcnn_debug_banded16_tables."""
    model = random_wide_model(channels, 64, f2, 32, 22)
    rc, table, exps = raw_tables(model)
    assert rc == table.nbytes == 4 * f2 * f2 * 2 * 64 * 16
    lib, _, fp = hook()
    fn = lib.srcnn_debug_banded16_tables
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.POINTER(C.c_uint16), C.POINTER(C.c_int)]
    want = np.zeros_like(table)
    wexps = (C.c_int * 2)()
    w1c, b1c, w2c = (np.ascontiguousarray(a.ravel()) for a in model[:3])
    assert fn(channels, f2, w1c.ctypes.data_as(fp), b1c.ctypes.data_as(fp), w2c.ctypes.data_as(fp),
              want.ctypes.data_as(C.POINTER(C.c_uint16)), wexps) == want.nbytes
    assert np.array_equal(table, want) and exps == (wexps[0], wexps[1])
    assert table.any()


@pytest.mark.parametrize("n1,n2", WIDTHS)
def test_a_model_that_cannot_be_scaled_is_refused(n1, n2):
    w1, b1, w2, b2, w3, b3 = random_wide_model(1, n1, 3, n2, 23)
    bad = w2.copy()
    bad[n2 - 1, n1 - 1, 1, 1] = np.inf
    assert raw_tables((w1, b1, bad, b2, w3, b3))[0] == S.ERR_STATE
    bad1 = b1.copy()
    bad1[n1 - 1] = np.nan
    assert raw_tables((w1, bad1, w2, b2, w3, b3))[0] == S.ERR_STATE
    tiny = (w2 * np.float32(1e-30)) * np.float32(1e-8)          # max |W2| near 2^-130: its scale 2^e2 is beyond float32's range
    assert np.abs(tiny).max() > 0 and raw_tables((w1, b1, tiny, b2, w3, b3))[0] == S.ERR_STATE
    assert raw_tables((w1, b1, w2, b2, w3, b3))[0] > 0


def test_the_hook_rejects_other_widths():
    _, fn, fp = hook()
    z = np.zeros(128 * 128 * 25, np.float32)
    exps = (C.c_int * 2)()
    p = z.ctypes.data_as(fp)
    for channels, n1p, n2p, f2 in [(1, 100, 64, 3), (1, 128, 40, 3), (2, 128, 64, 3), (1, 128, 64, 2), (1, 256, 64, 3)]:
        assert fn(channels, n1p, n2p, f2, p, p, p, 255.0, None, exps) == S.ERR_INVALID
    assert fn(1, 128, 64, 3, p, p, p, 0.0, None, exps) == S.ERR_INVALID


# ---- 3: the arithmetic ----------------------------------------------------------------------------------------------------
def rtz_f16(a):
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(h, np.float16(0)), h)


def split_model(x, model, key, padding, terms):
    """x [C, h, w] u8 -> the values before truncation [C, h, w] (float32 layers 1 and 3, split layer 2 over the padded widths;
    terms = 1: hi * hi only)."""
    pm, (chans, n1p, n2p, f2) = padded(model)
    w1, b1, _, b2, w3, b3 = pm
    r2 = (f2 - 1) // 2
    e1, e2, wh, wl = host_tables(model, key)

    def pad(t, r):
        return t if r == 0 else F.pad(t, (r,) * 4, mode="replicate" if padding == "replicate" else "constant")

    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    m1 = F.relu(F.conv2d(pad(t32(x)[None], 4), t32(w1), t32(b1)))[0].numpy()
    a = m1 * np.float32(2.0 ** e1)
    assert a.max() < 2.0 ** 15
    a_hi = rtz_f16(a)
    a_lo = (a - a_hi.astype(np.float32)).astype(np.float16)
    assert (a_lo >= 0).all() and np.isfinite(a_lo).all()
    conv = lambda act, w: F.conv2d(pad(t64(act.astype(np.float64))[None], r2), t64(w))[0].numpy()
    acc = conv(a_hi, wh)
    if terms == 3:
        acc = acc + conv(a_hi, wl) + conv(a_lo, wh)
    m2 = np.maximum(acc.astype(np.float32).astype(np.float64) * 2.0 ** -(e1 + e2) + np.asarray(b2, np.float64)[:, None, None], 0)
    pre = F.conv2d(pad(t32(m2)[None], 2), t32(w3), t32(b3))
    return pre[0].numpy().astype(np.float64)


def planes(channels):
    x = synth_color(W, H, frame=1) if channels == 3 else synth_luma(W, H, frame=1)[:, :, None]
    return np.ascontiguousarray(np.moveaxis(x, 2, 0))


@functools.lru_cache(maxsize=None)
def case(channels, n1, n2, f2, padding, terms=3):
    """(error of the split model against float64, tolerance) of one seeded model on the 130 x 70 image."""
    model = random_wide_model(channels, n1, f2, n2, 24)
    x = planes(channels)
    ref = forward(x, model, padding)
    n1p, n2p = padded_widths(n1, n2)
    err = np.abs(split_model(x, model, ("a", channels, n1, n2, f2), padding, terms) - ref).max()
    return err, pre_tolerance(ref) * max(n1p // 64, n2p // 32)


@pytest.mark.parametrize("padding", ["replicate", "zero"])
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_split_arithmetic_meets_the_wide_tolerance_128_64(channels, f2, padding):
    err, tol = case(channels, 128, 64, f2, padding)
    print(f"128/64 {channels}ch 9-{f2}-5 {padding}: split error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


@pytest.mark.parametrize("n1,n2", [(128, 32), (64, 64), (100, 40)])
def test_split_arithmetic_meets_the_wide_tolerance_other_widths(n1, n2):
    err, tol = case(1, n1, n2, 3, "zero")
    print(f"{n1}/{n2} 9-3-5 zero: split error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


@pytest.mark.parametrize("channels,f2", [(1, 3), (3, 3), (3, 5)])
def test_hi_parts_alone_miss_the_tolerance(channels, f2):
    """Plain f16 operands (no lo parts) are outside the contract, under the doubled tolerance of 128 / 64 too: what the split
    buys.  Measured for this seed (hi-only error against the tolerance of 0.01): 1 channel 9-3-5 0.0102, 3 channels 9-3-5 0.0106
    and 9-5-5 0.0139 miss it; 1 channel 9-5-5 stays INSIDE (0.0071) and is left out of this list -- the tolerance is twice that
    of 64 / 32 while the generator scales W2 by sqrt(64 / 128), so the margin of tests/test_banded16_cpu.py is gone, and the
    tolerance is not tightened to bring it back.  (f2 = 1 sums 128 products, not 1152 or 3200: not asserted, as for 64 / 32.)"""
    err, tol = case(channels, 128, 64, f2, "replicate", terms=1)
    print(f"128/64 {channels}ch 9-{f2}-5: hi-only error {err:.3g}, tolerance {tol:.3g}")
    assert err > tol


def test_the_numpy_model_restates_the_one_of_banded16_at_64_32():
    """The generalised model on a 64 / 32 model is tests/test_banded16_cpu.py's: same table, same exponents, same values."""
    import test_banded16_cpu as T
    plain = random_model(3, 1)
    y = synth_luma(W, H, frame=1)
    want = T.split_model(y[None], plain, "replicate", 3)[0]
    w1, b1, w2, b2, w3, b3 = as_model(*plain)
    model = (w1[:, None], b1, w2, b2, w3[None], np.array([b3], np.float32))
    got = split_model(y[None], model, ("r", 3), "replicate", 3)[0]
    assert np.array_equal(got, want)


# ---- 4: the device code of the wide forms (srcnn_spatial_kernels.hip) -----------------------------------------------------
def l2h_lds_bytes(f2):
    """spatial_l2h_lds_bytes(f2) (srcnn_kernels.h): four window planes [plane][hi, lo] and one step's A fragments."""
    r = (f2 - 1) // 2
    ps = ((16 + 2 * r) * (64 + 2 * r) + 7) // 8 * 8 + 4
    return (4 * ps + f2 * f2 * 2 * 64) * 16


def test_the_units_kernels():
    ks = L.kernels(L.L2H_WIDE)
    assert len(ks) == 6 and len({k[0] for k in ks}) == 6
    forms = sorted(re.search(L.L2H_WIDE, k[0]).groups() for k in ks)
    assert forms == sorted((f, z) for f in "135" for z in "01")          # f2 = 1, 3, 5 x replicate, zero
    for name, desc, body in ks:
        assert L.private_bytes(desc) == 0, f"{name} has a private segment"
        assert "scratch_" not in body, name
        assert L.mfma_kinds(body) == {"v_mfma_f32_32x32x16_f16"}, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 512
        # all LDS is dynamic: the launcher's constant below is the whole of it
        assert L.static_lds_bytes(desc) == 0


def test_the_launchers_lds_sizes_are_those_of_spatial_l2h_kernel():
    """The launcher asks for spatial_l2h_lds_bytes(f2) (srcnn_kernels.h; the kernel static_asserts that this is its layout's size):
    66 / 93 / 135 KiB, inside the 160 KiB of a gfx950 CU.  One function, used by the one kernel and the one launcher."""
    lib = C.CDLL(str(S.tuning_library_path()))
    lib.srcnn_debug_wide16_lds_bytes.restype = C.c_int
    lib.srcnn_debug_wide16_lds_bytes.argtypes = [C.c_int]
    got = [lib.srcnn_debug_wide16_lds_bytes(f2) for f2 in (1, 3, 5)]
    assert got == [l2h_lds_bytes(f2) for f2 in (1, 3, 5)]
    assert [round(b / 1024) for b in got] == [66, 93, 135] and max(got) <= 160 * 1024
    assert lib.srcnn_debug_wide16_lds_bytes(7) == S.ERR_INVALID
    src, header = (B.CSRC / L.UNIT).read_text(), (B.CSRC / "srcnn_kernels.h").read_text()
    assert "const size_t lds = spatial_l2h_lds_bytes(f);" in src and "== spatial_l2h_lds_bytes(F2)" in src
    # the figures are the header's one pair of functions, for the tile the kernel unit states
    assert "(((16 + 2 * r2) * (64 + 2 * r2) + 7) / 8) * 8 + 4" in header
    assert "((size_t)4 * spatial_l2h_ps((f2 - 1) / 2) + (size_t)f2 * f2 * 2 * 64) * 16" in header
    for fn in (r"\w+_l2h_ps\(int", r"\w+_l2h_lds_bytes\(int"):
        assert len(re.findall(fn, header + src)) == 1, fn
    assert "constexpr int SL2_COLS = 64, SL2_ROWS = 16," in src and "PS >= WR * WC" in src
