"""Row stripes of a colour model and of float planes (srcnn_model_color_rows*_dev, srcnn_model_rows*_f32_dev,
srcnn_model_color_striped*, srcnn_model_striped_f32*) without a GPU: the ABI, the argument checks that need no device, the
Python bindings' validation, and the device code of the twelve stripe forms of layer 1."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spatial_listing as L
import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["srcnn_model_color_rows_dev", "srcnn_model_color_rows_halo_dev", "srcnn_model_color_striped_dev",
               "srcnn_model_color_striped", "srcnn_model_rows_f32_dev", "srcnn_model_rows_halo_f32_dev",
               "srcnn_model_striped_f32_dev", "srcnn_model_striped_f32"]


@pytest.fixture(scope="module")
def lib():
    B.build()
    return S.load_library()


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_eight_entry_points(lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srcnn_amd.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in srcnn_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in S.ABI_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    assert set(NEW_SYMBOLS) <= {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert lib.srcnn_abi_version() == 1                      # a plain addition: no version bump


def test_null_contexts_are_invalid(lib):
    assert lib.srcnn_model_color_rows_dev(None, None, 0, 0, None, 0, 0, 4, 4, 0, 4, None) == S.ERR_INVALID
    assert lib.srcnn_model_color_rows_halo_dev(None, None, 0, 0, 4, None, None, 0, None, 0, 0, 4, 4, 0, 4, None) == S.ERR_INVALID
    assert lib.srcnn_model_rows_f32_dev(None, None, 0, 0, 0, None, 0, 0, 0, 4, 4, 0, 4) == S.ERR_INVALID
    assert lib.srcnn_model_rows_halo_f32_dev(None, None, 0, 0, 0, 4, None, None, 0, 0, None, 0, 0, 0, 4, 4, 0, 4) == S.ERR_INVALID
    img, x = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.float32)
    u8p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    one_null = (C.c_void_p * 1)(None)
    for ctxs, n in ((None, 1), (one_null, 1), (one_null, 0)):
        assert lib.srcnn_model_color_striped(ctxs, n, img.ctypes.data_as(u8p), 12, img.ctypes.data_as(u8p), 12, 4, 4) == S.ERR_INVALID
        assert lib.srcnn_model_color_striped_dev(ctxs, n, None, 12, None, 12, 4, 4) == S.ERR_INVALID
        assert lib.srcnn_model_striped_f32(ctxs, n, x.ctypes.data_as(f32p), 4, 0, x.ctypes.data_as(f32p), 4, 0, 4, 4) == S.ERR_INVALID
        assert lib.srcnn_model_striped_f32_dev(ctxs, n, None, 4, 0, None, 4, 0, 4, 4) == S.ERR_INVALID


# ---- the Python bindings validate before any call into the library --------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


def _shell_context():
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = _NoCall(), None
    return ctx


def test_colour_stripe_bindings_reject_bad_geometry_before_the_library():
    ctx = _shell_context()
    ok = dict(d_src=1, src_stride=600, src_row0=2, d_dst=2, dst_stride=600, dst_row0=10, width=200, height=61, row_begin=10, row_end=37)
    for bad in (dict(row_begin=37), dict(row_end=62), dict(row_begin=-1, src_row0=0, dst_row0=0), dict(src_stride=599),
                dict(src_stride=200), dict(dst_stride=599), dict(width=0), dict(height=0), dict(src_row0=11), dict(dst_row0=11),
                dict(src_row0=-1)):
        with pytest.raises(ValueError):
            ctx.model_color_rows_dev(**{**ok, **bad})
    halo = dict(ok, src_row0=10, src_rows=27, d_halo_top=3, d_halo_bot=4, halo_stride=600)
    for bad in (dict(src_rows=0), dict(src_rows=52), dict(halo_stride=599), dict(row_end=9), dict(dst_row0=12)):
        with pytest.raises(ValueError):
            ctx.model_color_rows_halo_dev(**{**halo, **bad})
    # good geometry is handed on: the shell's library is what stops the call
    with pytest.raises(AssertionError, match="srcnn_model_color_rows_dev"):
        ctx.model_color_rows_dev(**ok)
    with pytest.raises(AssertionError, match="srcnn_model_color_rows_halo_dev"):
        ctx.model_color_rows_halo_dev(**halo)


def test_float_stripe_bindings_reject_bad_geometry_before_the_library():
    ctx = _shell_context()
    ok = dict(d_src=1, src_stride=200, src_ch_pitch=20000, src_row0=2, d_dst=2, dst_stride=200, dst_ch_pitch=20000, dst_row0=10,
              width=200, height=61, row_begin=10, row_end=37)
    for bad in (dict(row_begin=37), dict(row_end=62), dict(src_stride=199), dict(dst_stride=100), dict(width=0), dict(height=0),
                dict(src_row0=11), dict(dst_row0=11), dict(src_row0=-1), dict(src_ch_pitch=-1), dict(dst_ch_pitch=-4)):
        with pytest.raises(ValueError):
            ctx.model_rows_f32_dev(**{**ok, **bad})
    halo = dict(ok, src_row0=10, src_rows=27, d_halo_top=3, d_halo_bot=4, halo_stride=200, halo_ch_pitch=4000)
    for bad in (dict(src_rows=0), dict(src_rows=52), dict(halo_stride=199), dict(row_end=9), dict(dst_row0=12), dict(halo_ch_pitch=-1)):
        with pytest.raises(ValueError):
            ctx.model_rows_halo_f32_dev(**{**halo, **bad})
    with pytest.raises(AssertionError, match="srcnn_model_rows_f32_dev"):
        ctx.model_rows_f32_dev(**ok)
    with pytest.raises(AssertionError, match="srcnn_model_rows_halo_f32_dev"):
        ctx.model_rows_halo_f32_dev(**halo)


def test_striped_bindings_reject_mismatched_shapes_before_the_library(monkeypatch):
    monkeypatch.setattr(S, "load_library", lambda: _NoCall())
    ctxs = [_shell_context(), _shell_context()]
    img = np.zeros((61, 200, 3), np.uint8)
    for bad_dst in (np.zeros((61, 199, 3), np.uint8), np.zeros((60, 200, 3), np.uint8)):
        with pytest.raises(ValueError):
            S.model_color_striped(ctxs, img, dst=bad_dst)
    for bad in (img.astype(np.float32), img[0], img[:, :, 0]):
        with pytest.raises(TypeError):
            S.model_color_striped(ctxs, bad)
    with pytest.raises(TypeError):
        S.model_color_striped(ctxs, img, dst=np.zeros((61, 200, 3), np.float32))       # a wrongly typed output
    with pytest.raises(ValueError):
        S.model_color_striped(ctxs, np.zeros((61, 400, 3), np.uint8)[:, ::2])          # pixels not packed
    ro = np.zeros((61, 200, 3), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        S.model_color_striped(ctxs, img, dst=ro)
    with pytest.raises(ValueError):
        S.model_color_striped([], img)
    with pytest.raises(ValueError):
        S.model_color_striped_dev(ctxs, [1], 600, [2, 3], 600, 200, 61)          # one stripe for two contexts
    with pytest.raises(ValueError):
        S.model_color_striped_dev(ctxs, [1, 2], 600, [3], 600, 200, 61)
    with pytest.raises(ValueError):
        S.model_color_striped_dev(ctxs, [1, 2], 599, [3, 4], 600, 200, 61)       # a stride below the row of 3-byte pixels
    with pytest.raises(ValueError):
        S.model_color_striped_dev(ctxs, [1, 2], 600, [3, 4], 200, 200, 61)
    with pytest.raises(ValueError):
        S.model_color_striped_dev(ctxs, [1, 2], 600, [3, 4], 600, 0, 61)
    with pytest.raises(ValueError):
        S.model_color_striped_dev([], [], 600, [], 600, 200, 61)
    with pytest.raises(AssertionError, match="srcnn_model_color_striped_dev"):
        S.model_color_striped_dev(ctxs, [1, 2], 600, [3, 4], 600, 200, 61)
    with pytest.raises(AssertionError, match="srcnn_model_color_striped"):
        S.model_color_striped(ctxs, img)

    x = np.zeros((3, 61, 200), np.float32)
    for bad_out in (np.zeros((3, 61, 199), np.float32), np.zeros((61, 200), np.float32)):
        with pytest.raises(ValueError):
            S.model_striped_f32(ctxs, x, out=bad_out)
    for bad in (x.astype(np.float64), x[0, 0], x[None]):
        with pytest.raises(TypeError):
            S.model_striped_f32(ctxs, bad)
    with pytest.raises(TypeError):
        S.model_striped_f32(ctxs, x, out=np.zeros((3, 61, 200), np.uint8))
    with pytest.raises(ValueError):
        S.model_striped_f32(ctxs, np.zeros((3, 61, 400), np.float32)[:, :, ::2])    # rows not contiguous
    with pytest.raises(ValueError):
        S.model_striped_f32(ctxs, np.zeros((2, 61, 200), np.float32))                # 2 channels
    rof = np.zeros((3, 61, 200), np.float32)
    rof.flags.writeable = False
    with pytest.raises(ValueError):
        S.model_striped_f32(ctxs, x, out=rof)
    with pytest.raises(ValueError):
        S.model_striped_f32([], x)
    with pytest.raises(ValueError):
        S.model_striped_f32_dev(ctxs, [1], 200, 8000, [2, 3], 200, 8000, 200, 61)
    with pytest.raises(ValueError):
        S.model_striped_f32_dev(ctxs, [1, 2], 199, 8000, [3, 4], 200, 8000, 200, 61)
    with pytest.raises(ValueError):
        S.model_striped_f32_dev(ctxs, [1, 2], 200, -1, [3, 4], 200, 8000, 200, 61)
    with pytest.raises(ValueError):
        S.model_striped_f32_dev([], [], 200, 0, [], 200, 0, 200, 61)
    with pytest.raises(AssertionError, match="srcnn_model_striped_f32_dev"):
        S.model_striped_f32_dev(ctxs, [1, 2], 200, 8000, [3, 4], 200, 8000, 200, 61)
    # any row / channel stride goes through: a (C, H, W) view of a padded parent, and an (H, W) plane
    parent = np.zeros((3, 70, 216), np.float32)
    with pytest.raises(AssertionError, match="srcnn_model_striped_f32"):
        S.model_striped_f32(ctxs, parent[:, 4:65, 8:208])
    with pytest.raises(AssertionError, match="srcnn_model_striped_f32"):
        S.model_striped_f32(ctxs, x[0])


# ---- the device code ------------------------------------------------------------------------------------------------------
def test_the_unit_holds_the_twelve_new_kernels_without_scratch_memory():
    found = L.kernels("L1RowsCF")
    names = [n for n, _, _ in found]
    assert len(names) == 12 and len(set(names)) == 12, names
    assert names == [n for n, _, _ in L.kernels(L.L1_ROWS_CF)]
    assert all("spatial_l1_kernel" in n and "L1RowsCF" in n for n in names), names
    # (C, In) x ZERO x Scale: In follows Scale in the mangled name -- NoScale is NS_7NoScaleE, float is f; bytes h, floats f
    forms = {}
    for n in names:
        m = re.search(r"spatial_l1_kernelILi(\d)ELb([01])E(NS_7NoScaleE|f)([hf])JNS_8L1RowsCFE", n)
        assert m, n
        forms.setdefault((int(m.group(1)), m.group(4)), set()).add((m.group(2), m.group(3)))
    assert set(forms) == {(3, "h"), (1, "f"), (3, "f")}
    assert all(len(v) == 4 for v in forms.values()), forms
    for name, desc, _ in found:
        assert L.private_bytes(desc) == 0, name
        # one float plane: the window and the layer-1 table, all static, 16 x 136 x 4 + 82 x 64 x 4 bytes as the whole-image
        # form; three channels: all dynamic (68 KiB bytes, 87 KiB floats), so no static LDS shifts it
        lds = L.static_lds_bytes(desc)
        assert lds == (29696 if "kernelILi1E" in name else 0), (name, lds)
    assert sum("kernelILi1E" in n for n in names) == 4


def test_the_new_kernels_run_on_the_f32_mfma_only():
    found = L.kernels("L1RowsCF")
    for name, _, body in found:
        assert L.mfma_kinds(body) == {"v_mfma_f32_32x32x2_f32"}, (name, L.mfma_kinds(body))
    assert len(found) == 12


def test_one_unit_holds_every_form_and_no_launcher_is_weak():
    """What the side units, the weak launchers and the launchers handed over by constructors stood for: the kernel set of the
    banded path is exactly the one it was, the wide forms of layers 2 and 3 included, and the host layer depends on no optional
    symbol (tests/checks/san_host.cpp links it against three stubs)."""
    names = [n for n, _, _ in L.kernels()]
    assert len(names) == 79 and len(set(names)) == 79, names
    families = [("split3_kernel", 1), (L.L1_BYTES, 8), (L.L1_ROWS, 4), (L.L1_ROWS_CF, 12), (L.L1_FLOATS, 8),
                (L.L2, 6), (L.L2H, 6), (L.L3_BYTES, 6), (L.L3_FLOATS, 4), (L.L2_WIDE, 6), (L.L2H_WIDE, 6), (L.L3_WIDE, 12)]
    picked = []
    for pattern, count in families:
        family = [n for n, _, _ in L.kernels(pattern)]
        assert len(family) == count, (pattern, family)
        picked += family
    assert sorted(picked) == sorted(names)                     # every kernel is in exactly one family
    header = (B.CSRC / "srcnn_kernels.h").read_text()
    assert "weak" not in header
    assert not re.search(r"set_\w*launcher", header) and "Launchers" not in header       # nothing is handed over at load time
    assert "__attribute__((constructor))" not in (B.CSRC / L.UNIT).read_text()
    assert len(re.findall(r"^hipError_t launch_spatial_\w+\(", header, re.M)) == 3
    units = [u[0] for u in B.UNITS]
    assert units.count(L.UNIT) == 1
    for gone in ("srcnn_spatial_f32.hip", "srcnn_spatial_rows.hip", "srcnn_spatial_rows_cf.hip", "srcnn_wide_kernels.hip",
                 "srcnn_wide16_kernels.hip"):
        assert gone not in units and not (B.CSRC / gone).exists()
