"""Row stripes of every 1-channel model (srcnn_model_halo_rows, srcnn_model_rows_dev, srcnn_model_rows_halo_dev,
srcnn_model_striped, srcnn_model_striped_dev) without a GPU: the ABI, the argument checks that need no device, the Python
bindings' validation, and the device code of the stripe forms of layer 1."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spatial_listing as L
import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["srcnn_model_halo_rows", "srcnn_model_rows_dev", "srcnn_model_rows_halo_dev", "srcnn_model_striped",
               "srcnn_model_striped_dev"]


@pytest.fixture(scope="module")
def lib():
    B.build()
    return S.load_library()


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_stripe_entry_points(lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srcnn_amd.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in srcnn_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in S.ABI_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    assert set(NEW_SYMBOLS) <= {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert lib.srcnn_abi_version() == 1                      # a plain addition: no version bump


def test_null_contexts_and_bad_arguments(lib):
    import ctypes as C
    assert lib.srcnn_model_halo_rows(None) == S.ERR_INVALID
    assert lib.srcnn_model_rows_dev(None, None, 0, 0, None, 0, 0, 4, 4, 0, 4, None) == S.ERR_INVALID
    assert lib.srcnn_model_rows_halo_dev(None, None, 0, 0, 4, None, None, 0, None, 0, 0, 4, 4, 0, 4, None) == S.ERR_INVALID
    buf = np.zeros((4, 4), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    assert lib.srcnn_model_striped(None, 1, buf.ctypes.data_as(u8p), 4, buf.ctypes.data_as(u8p), 4, 4, 4) == S.ERR_INVALID
    assert lib.srcnn_model_striped_dev(None, 1, None, 4, None, 4, 4, 4) == S.ERR_INVALID
    one_null = (C.c_void_p * 1)(None)
    assert lib.srcnn_model_striped(one_null, 1, buf.ctypes.data_as(u8p), 4, buf.ctypes.data_as(u8p), 4, 4, 4) == S.ERR_INVALID
    assert lib.srcnn_model_striped_dev(one_null, 1, None, 4, None, 4, 4, 4) == S.ERR_INVALID
    assert lib.srcnn_model_striped(one_null, 0, buf.ctypes.data_as(u8p), 4, buf.ctypes.data_as(u8p), 4, 4, 4) == S.ERR_INVALID


# ---- the Python bindings validate before any call into the library --------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


def _shell_context():
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = _NoCall(), None
    return ctx


def test_stripe_bindings_reject_bad_geometry_before_the_library():
    ctx = _shell_context()
    ok = dict(d_src=1, src_stride=200, src_row0=2, d_dst=2, dst_stride=200, dst_row0=10, width=200, height=61, row_begin=10, row_end=37)
    for bad in (dict(row_begin=37), dict(row_end=62), dict(row_begin=-1, src_row0=0, dst_row0=0), dict(src_stride=199),
                dict(dst_stride=100), dict(width=0), dict(height=0), dict(src_row0=11), dict(dst_row0=11), dict(src_row0=-1)):
        with pytest.raises(ValueError):
            ctx.model_rows_dev(**{**ok, **bad})
    halo = dict(ok, src_row0=10, src_rows=27, d_halo_top=3, d_halo_bot=4, halo_stride=200)
    for bad in (dict(src_rows=0), dict(src_rows=52), dict(halo_stride=199), dict(row_end=9), dict(dst_row0=12)):
        with pytest.raises(ValueError):
            ctx.model_rows_halo_dev(**{**halo, **bad})
    # good geometry is handed on: the shell's library is what stops the call
    with pytest.raises(AssertionError, match="srcnn_model_rows_dev"):
        ctx.model_rows_dev(**ok)
    with pytest.raises(AssertionError, match="srcnn_model_rows_halo_dev"):
        ctx.model_rows_halo_dev(**halo)
    with pytest.raises(AssertionError, match="srcnn_model_halo_rows"):
        ctx.model_halo_rows()


def test_striped_bindings_reject_mismatched_shapes_before_the_library(monkeypatch):
    monkeypatch.setattr(S, "load_library", lambda: _NoCall())
    ctxs = [_shell_context(), _shell_context()]
    y = np.zeros((61, 200), np.uint8)
    with pytest.raises(ValueError):
        S.model_striped(ctxs, y, dst=np.zeros((61, 199), np.uint8))
    with pytest.raises(ValueError):
        S.model_striped(ctxs, y, dst=np.zeros((60, 200), np.uint8))
    with pytest.raises(TypeError):
        S.model_striped(ctxs, y.astype(np.float32))
    with pytest.raises(TypeError):
        S.model_striped(ctxs, y[0])
    with pytest.raises(ValueError):
        S.model_striped(ctxs, np.zeros((61, 400), np.uint8)[:, ::2])
    ro = np.zeros((61, 200), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        S.model_striped(ctxs, y, dst=ro)
    with pytest.raises(ValueError):
        S.model_striped([], y)
    with pytest.raises(ValueError):
        S.model_striped_dev(ctxs, [1], 200, [2, 3], 200, 200, 61)          # one stripe for two contexts
    with pytest.raises(ValueError):
        S.model_striped_dev(ctxs, [1, 2], 200, [3], 200, 200, 61)
    with pytest.raises(ValueError):
        S.model_striped_dev(ctxs, [1, 2], 199, [3, 4], 200, 200, 61)
    with pytest.raises(ValueError):
        S.model_striped_dev(ctxs, [1, 2], 200, [3, 4], 200, 0, 61)
    with pytest.raises(AssertionError, match="srcnn_model_striped_dev"):
        S.model_striped_dev(ctxs, [1, 2], 200, [3, 4], 200, 200, 61)
    with pytest.raises(AssertionError, match="srcnn_model_striped"):
        S.model_striped(ctxs, y)


# ---- the device code ------------------------------------------------------------------------------------------------------
def test_the_stripe_unit_holds_the_four_new_kernels_without_scratch_memory():
    found = L.kernels("L1RowsE")
    names = [n for n, _, _ in found]
    assert len(names) == 4 and len(set(names)) == 4, names
    assert names == [n for n, _, _ in L.kernels(L.L1_ROWS)]
    # one byte channel, the row source in the argument pack: replicate, zero x f32, split map
    assert all("spatial_l1_kernelILi1E" in n and "L1Rows" in n for n in names), names
    assert sum("Lb1E" in n for n in names) == 2 and sum("NoScale" in n for n in names) == 2
    for name, desc, _ in found:
        assert L.private_bytes(desc) == 0, name
        # the window and the layer-1 table, all static: 16 x 136 x 4 + 82 x 64 x 4 bytes, as the whole-image 1-channel form
        assert L.static_lds_bytes(desc) == 29696, name


def test_the_stripe_kernels_run_on_the_f32_mfma_only():
    found = L.kernels("L1RowsE")
    for name, _, body in found:
        assert L.mfma_kinds(body) == {"v_mfma_f32_32x32x2_f32"}, (name, L.mfma_kinds(body))
    assert len(found) == 4
