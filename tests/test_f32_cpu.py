"""The float image path (srcnn_forward_f32, srcnn_forward_f32_dev, srcnn_set_input_range, srcnn_cpp_amd.torch_api) without a GPU:
the ABI, the range setting's argument check, the Python bindings' validation, the host side of SRCNN_MODE_BANDED16 for a range
other than 255 (through the tuning library's hook), a numpy model of the split arithmetic on float inputs in [0, 1], and the
device code of the new kernels."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatial_listing as L
import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd.synth import synth_luma
from color_reference import random_color_model, synth_color, torch_forward_color
from spatial_reference import as_model, pre_tolerance, random_model, torch_forward
from zero_pad_reference import torch_forward_zero

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["srcnn_forward_f32", "srcnn_forward_f32_dev", "srcnn_set_input_range", "srcnn_get_input_range"]
W, H = 130, 70


def scaled_tolerance(ref, r):
    """The project's tolerance for 0..255 data, carried to data of range r by homogeneity."""
    return pre_tolerance(np.asarray(ref) * 255.0 / r) * r / 255.0


@pytest.fixture(scope="module")
def lib():
    B.build()
    return S.load_library()


@pytest.fixture(scope="module")
def tuning():
    B.build()
    return C.CDLL(str(S.tuning_library_path()))


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_float_entry_points(lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srcnn_amd.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in srcnn_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in S.ABI_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    assert set(NEW_SYMBOLS) <= {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert lib.srcnn_abi_version() == 1                      # a plain addition: no version bump


def test_null_context(lib):
    assert lib.srcnn_set_input_range(None, 1.0) == S.ERR_INVALID
    assert lib.srcnn_get_input_range(None) == float(S.ERR_INVALID)
    assert lib.srcnn_forward_f32(None, None, 0, 0, None, 0, 0, 4, 4) == S.ERR_INVALID
    assert lib.srcnn_forward_f32_dev(None, None, 0, 0, 0, None, 0, 0, 0, 4, 4, 1) == S.ERR_INVALID


def set_range_on_a_bare_context(tuning, r):
    """(return code, the setting afterwards) of srcnn_set_input_range on a context that was never bound to a device."""
    fn = tuning.srcnn_debug_set_input_range
    fn.restype, fn.argtypes = C.c_int, [C.c_float, C.POINTER(C.c_float)]
    after = C.c_float(-1.0)
    return fn(r, C.byref(after)), after.value


def test_input_range_default_and_argument_check(tuning):
    rc, after = set_range_on_a_bare_context(tuning, 1.0)
    assert rc == 0 and after == 1.0
    rc, after = set_range_on_a_bare_context(tuning, 1023.0)
    assert rc == 0 and after == 1023.0
    for bad in (0.0, -0.0, -1.0, -255.0, float("nan"), float("inf"), float("-inf")):
        rc, after = set_range_on_a_bare_context(tuning, bad)
        assert rc == S.ERR_INVALID, bad
        assert after == 255.0, "a refused value leaves the default of 255"


# ---- the Python bindings validate before any call into the library --------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with a bad array")


def _shell_context():
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = _NoCall(), None
    return ctx


def test_numpy_binding_rejects_bad_arrays_before_the_library():
    ctx = _shell_context()
    f32 = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(TypeError):
        ctx.forward_f32(np.zeros((8, 8), np.float64))
    with pytest.raises(TypeError):
        ctx.forward_f32(np.zeros((8, 8), np.uint8))
    with pytest.raises(TypeError):
        ctx.forward_f32(f32(8))                               # 1-D
    with pytest.raises(TypeError):
        ctx.forward_f32(f32(1, 1, 1, 8, 8))                   # 5-D
    with pytest.raises(TypeError):
        ctx.forward_f32([[0.0] * 8] * 8)                      # not an array
    with pytest.raises(ValueError):
        ctx.forward_f32(f32(8, 16)[:, ::2])                   # innermost dimension not contiguous
    with pytest.raises(ValueError):
        ctx.forward_f32(np.moveaxis(f32(8, 8, 3), 2, 0))      # interleaved pixels seen as (3, H, W)
    with pytest.raises(ValueError):
        ctx.forward_f32(f32(16, 8)[::-1])                     # negative row stride
    with pytest.raises(ValueError):
        ctx.forward_f32(f32(0, 8))
    with pytest.raises(ValueError):
        ctx.forward_f32(f32(2, 8, 8))                         # 2 channels: no such model
    with pytest.raises(ValueError):
        ctx.forward_f32(f32(8, 8), out=f32(8, 7))
    with pytest.raises(ValueError):
        ctx.forward_f32(f32(3, 8, 8), out=f32(1, 3, 8, 8))
    with pytest.raises(TypeError):
        ctx.forward_f32(f32(8, 8), out=np.zeros((8, 8), np.uint8))
    ro = f32(8, 8)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        ctx.forward_f32(f32(8, 8), out=ro)
    # a padded view passes the checks and is handed on with its strides: the shell's library is what stops the call
    with pytest.raises(AssertionError, match="srcnn_get_model_channels"):
        ctx.forward_f32(f32(2, 3, 8, 16)[:, :, :, :5])


def test_f32_planes_strides():
    a = np.zeros((2, 3, 8, 16), np.float32)[:, :, 1:7, 2:7]
    v = S._f32_planes(a, "x")
    assert v.shape == (2, 3, 6, 5) and [s // 4 for s in v.strides] == [3 * 8 * 16, 8 * 16, 16, 1]
    v = S._f32_planes(np.zeros((8, 16), np.float32)[:, :5], "x")
    assert v.shape == (1, 1, 8, 5) and v.strides[2] == 64


def test_torch_binding_rejects_bad_tensors_before_the_library():
    from srcnn_cpp_amd import torch_api as T
    call = T.CompiledModule(_shell_context(), 1, 0)           # no device: only the checks run
    with pytest.raises(ValueError, match="cuda"):
        call(torch.zeros(1, 1, 8, 8))                         # a CPU tensor
    with pytest.raises(ValueError, match="float32"):
        call(torch.zeros(1, 1, 8, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        call(torch.zeros(1, 1, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        call(np.zeros((1, 1, 8, 8), np.float32))
    # shape, channel count and strides are checked before the device, so CPU tensors show them
    with pytest.raises(ValueError, match="channel"):
        call(torch.zeros(1, 3, 8, 8))                         # a 3-channel tensor for a 1-channel module
    with pytest.raises(ValueError, match="channel"):
        T.CompiledModule(_shell_context(), 3, 0)(torch.zeros(1, 8, 8))
    with pytest.raises(ValueError, match="shape"):
        call(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros(1, 1, 8, 16)[:, :, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        T.CompiledModule(_shell_context(), 3, 0)(torch.zeros(2, 8, 8, 3).permute(0, 3, 1, 2))      # channels-last pixels
    with pytest.raises(ValueError, match="empty"):
        call(torch.zeros(1, 1, 0, 8))
    with pytest.raises(ValueError, match="MODE_MFMA"):
        T.compile_module(torch.nn.Identity(), mode=S.MODE_EXACT)
    with pytest.raises(ValueError, match="conv1"):
        T.compile_module(torch.nn.Identity())


# ---- SRCNN_MODE_BANDED16 for a range other than 255: e1 follows the range, the W2 table does not ---------------------------
def acc_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def l2h_channel(step, h, e):
    return 32 * (step >> 1) + acc_row(8 * (step & 1) + e, h)


def host_tables(tuning, model, r):
    """(return code, e1, e2, the table's uint16 words) of the library's host side for input range r."""
    w1, b1, w2 = (np.ascontiguousarray(np.asarray(a, np.float32).ravel()) for a in model[:3])
    channels = 3 if np.ndim(model[0]) == 4 else 1
    f2 = 1 if np.ndim(model[2]) == 2 else np.shape(model[2])[2]
    fn = tuning.srcnn_debug_banded16_tables_range
    fp, u16p = C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, fp, fp, fp, C.c_float, u16p, C.POINTER(C.c_int)]
    table = np.zeros(4 * f2 * f2 * 2 * 64 * 8, np.uint16)
    exps = (C.c_int * 2)()
    rc = fn(channels, f2, w1.ctypes.data_as(fp), b1.ctypes.data_as(fp), w2.ctypes.data_as(fp), r, table.ctypes.data_as(u16p), exps)
    return rc, exps[0], exps[1], table


def decode(table, f2):
    taps = f2 * f2
    t = table.view(np.float16).astype(np.float64).reshape(4, taps, 2, 64, 8)
    wh, wl = np.zeros((32, 64, taps)), np.zeros((32, 64, taps))
    for s in range(4):
        for h in range(2):
            for e in range(8):
                ci = l2h_channel(s, h, e)
                wh[:, ci, :] = t[s, :, 0, 32 * h:32 * h + 32, e].T
                wl[:, ci, :] = t[s, :, 1, 32 * h:32 * h + 32, e].T
    return wh.reshape(32, 64, f2, f2), wl.reshape(32, 64, f2, f2)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_e1_follows_the_range_and_the_w2_table_does_not(tuning, f2, channels):
    model = random_color_model(f2, 1) if channels == 3 else random_model(f2, 1)
    w1, b1 = np.asarray(model[0], np.float64), np.asarray(model[1], np.float64)
    sums = np.abs(w1).reshape(64, -1).sum(1)
    seen = {}
    for r in (1.0, 255.0, 1023.0, 1e-3, 65535.0):
        rc, e1, e2, table = host_tables(tuning, model, r)
        assert rc == table.nbytes
        bound = (r * sums + np.abs(b1)).max()
        assert 2.0 ** 14 <= bound * 2.0 ** e1 < 2.0 ** 15, (r, e1)
        assert e1 == 15 - (np.frexp(bound)[1])
        seen[r] = (e1, e2, table)
    assert seen[1.0][0] > seen[255.0][0] > seen[65535.0][0]           # a smaller range leaves room for a larger scale
    for r in seen:
        assert seen[r][1] == seen[255.0][1]
        assert np.array_equal(seen[r][2], seen[255.0][2]), f"the W2 table changed with the range ({r})"
    # the hook of the byte path is the range 255
    fn = tuning.srcnn_debug_banded16_tables
    fp, u16p = C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, fp, fp, fp, u16p, C.POINTER(C.c_int)]
    w1c, b1c, w2c = (np.ascontiguousarray(np.asarray(a, np.float32).ravel()) for a in model[:3])
    exps = (C.c_int * 2)()
    assert fn(channels, f2, w1c.ctypes.data_as(fp), b1c.ctypes.data_as(fp), w2c.ctypes.data_as(fp), None, exps) == seen[255.0][2].nbytes
    assert (exps[0], exps[1]) == seen[255.0][:2]


def test_the_hook_rejects_a_bad_range(tuning):
    model = random_model(3, 0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert host_tables(tuning, model, bad)[0] == S.ERR_INVALID


# ---- the split arithmetic on float inputs in [0, 1] ------------------------------------------------------------------------
def rtz_f16(a):
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(h, np.float16(0)), h)


def split_model_f32(tuning, x, model, padding, r):
    """x [C, h, w] float32 in the model's units, |x| <= r -> the values before truncation [C, h, w]: float32 layers 1 and 3,
    layer 2 as hi*hi + lo*hi + hi*lo on the library's own table and the exponents it makes for range r."""
    w1, b1, w2, b2, w3, b3 = model
    w1, w3 = np.asarray(w1, np.float32), np.asarray(w3, np.float32)
    chans = x.shape[0]
    f2 = 1 if np.ndim(w2) == 2 else w2.shape[2]
    r2 = (f2 - 1) // 2
    rc, e1, e2, table = host_tables(tuning, model, r)
    assert rc == table.nbytes
    wh, wl = decode(table, f2)

    def pad(t, k):
        return t if k == 0 else F.pad(t, (k,) * 4, mode="replicate" if padding == "replicate" else "constant")

    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    m1 = F.relu(F.conv2d(pad(t32(x)[None], 4), t32(w1.reshape(64, chans, 9, 9)), t32(b1)))[0].numpy()
    a = m1 * np.float32(2.0 ** e1)
    assert 2.0 ** 10 < a.max() < 2.0 ** 15                    # the range put the map where f16 resolves it
    a_hi = rtz_f16(a)
    a_lo = (a - a_hi.astype(np.float32)).astype(np.float16)
    assert np.isfinite(a_hi.astype(np.float32)).all() and np.isfinite(a_lo.astype(np.float32)).all()
    conv = lambda act, w: F.conv2d(pad(t64(act.astype(np.float64))[None], r2), t64(w))[0].numpy()
    acc = conv(a_hi, wh) + conv(a_hi, wl) + conv(a_lo, wh)
    m2 = np.maximum(acc.astype(np.float32).astype(np.float64) * 2.0 ** -(e1 + e2) + np.asarray(b2, np.float64)[:, None, None], 0)
    pre = F.conv2d(pad(t32(m2)[None], 2), t32(w3.reshape(chans, 32, 5, 5)), t32(np.atleast_1d(np.asarray(b3, np.float32))))
    return pre[0].numpy().astype(np.float64), e1


@pytest.mark.parametrize("padding", ["replicate", "zero"])
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_split_arithmetic_on_unit_range_input_meets_the_scaled_tolerance(tuning, f2, padding):
    """A model as trained on [0, 1] (weights and biases untouched), inputs synth / 255 as float32, range 1.

    Recorded (130x70, seed 1): the error against float64 is 4.4e-6 / 3.8e-6 / 7.7e-6 for f2 = 1 / 3 / 5 under replicate padding
    and 4.5e-6 / 3.9e-6 / 7.7e-6 under zero padding, against a scaled tolerance of 1.05e-3 / 1.18e-3 / 1.61e-3 (5e-3 * max|ref|
    / 255 with outputs up to 53 / 60 / 82); e1 is 12 with range 1, where the 255 of the byte path gives 5: with the byte path's
    scale the map of these inputs would sit 7 bits lower in f16's range."""
    model = random_model(f2, 1)
    x = (synth_luma(W, H, frame=1).astype(np.float32) / np.float32(255.0))
    ref = torch_forward(x, model) if padding == "replicate" else torch_forward_zero(x, model)
    got, e1 = split_model_f32(tuning, x[None], model, padding, 1.0)
    err, tol = np.abs(got[0] - ref).max(), scaled_tolerance(ref, 1.0)
    print(f"9-{f2}-5 {padding}: e1 {e1} (range 255: {host_tables(tuning, model, 255.0)[1]}), error {err:.3g}, tolerance {tol:.3g}, "
          f"max |ref| {np.abs(ref).max():.3g}")
    assert err <= tol


@pytest.mark.parametrize("f2", [1, 5])
def test_split_arithmetic_colour_and_ten_bit_range(tuning, f2):
    """A colour model on [0, 1] input with range 1, and a luma model on a 0..1023 plane with range 1023.

    Recorded: colour 9-1-5 / 9-5-5 error 7.9e-6 / 7.8e-6 against 1.65e-3 / 1.31e-3; 10-bit 2.7e-5 / 5.1e-5 against 2.0e-2
    (outputs up to 56 / 80, so the tolerance is its floor 5e-3 * 1023 / 255)."""
    cm = random_color_model(f2, 2)
    img = synth_color(W, H, frame=2).astype(np.float32) / np.float32(255.0)
    ref = torch_forward_color(img, cm, "zero")
    got, _ = split_model_f32(tuning, np.moveaxis(img, 2, 0), cm, "zero", 1.0)
    err, tol = np.abs(np.moveaxis(got, 0, 2) - ref).max(), scaled_tolerance(ref, 1.0)
    print(f"colour 9-{f2}-5: error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    model = random_model(f2, 2)
    y = ten_bit_plane(W, H)
    ref = torch_forward(y, model)
    got, _ = split_model_f32(tuning, y[None], model, "replicate", 1023.0)
    err, tol = np.abs(got[0] - ref).max(), scaled_tolerance(ref, 1023.0)
    print(f"10-bit 9-{f2}-5: error {err:.3g}, tolerance {tol:.3g}, max |ref| {np.abs(ref).max():.3g}")
    assert err <= tol


def ten_bit_plane(w, h):
    """A 0..1023 plane with non-integer values: the 8-bit test pattern times 1023 / 255, plus a quarter-step dither."""
    y = synth_luma(w, h, frame=3).astype(np.float32) * np.float32(1023.0 / 255.0)
    return np.clip(y + np.float32(0.25) * ((np.arange(w)[None] + np.arange(h)[:, None]) % 4).astype(np.float32) - 0.375, 0, 1023).astype(np.float32)


# ---- the device code ------------------------------------------------------------------------------------------------------
def float_kernels():
    """The whole-image float forms of layers 1 and 3 (the stripe forms of float planes carry L1RowsCF in their names)."""
    return L.kernels(L.L1_FLOATS), L.kernels(L.L3_FLOATS)


def test_the_float_unit_holds_the_twelve_new_kernels_without_scratch_memory():
    l1, l3 = float_kernels()
    assert len(l1) == 8                                             # 1, 3 channels x replicate, zero x f32, split map
    assert len(l3) == 4                                             # 1, 3 channels x replicate, zero
    assert not any("L1Rows" in name for name, _, _ in l1)
    assert len({name for name, _, _ in l1 + l3}) == 12
    for name, desc, _ in l1 + l3:
        assert L.private_bytes(desc) == 0, name
    # the colour layer-1 forms stage an f32 window beside the three tables: 3 * 82 * 64 * 4 + 3 * 16 * 136 * 4 bytes, dynamic
    # (no static LDS ahead of it), i.e. one workgroup per CU
    for name, desc, _ in l1 + l3:
        if "spatial_l1_kernelILi3" in name:
            assert L.static_lds_bytes(desc) == 0, name
    assert sum("spatial_l1_kernelILi3" in name for name, _, _ in l1) == 4


def test_the_float_kernels_run_on_the_f32_mfma_and_store_no_byte():
    l1, l3 = float_kernels()
    for name, _, body in l1 + l3:
        assert L.mfma_kinds(body) == {"v_mfma_f32_32x32x2_f32"}, (name, L.mfma_kinds(body))
        assert "global_store_byte" not in body and "global_load_ubyte" not in body, name
    assert len(l1 + l3) == 12
