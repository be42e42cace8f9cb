"""CPU tests of the antialiased cubic resize (srcnn_cubic_aa_f32_taps, srcnn_resize_cubic_aa_*): no device.
1. the float64 formula (tests/resize_aa_reference.py) against torch's own antialiased result on float64 tensors;
2. srcnn_cubic_aa_f32_taps -- the one table builder, also what the kernels run on -- against the numpy table, bit for bit, its
   invariants, the query form and the refusals;
3. the float32 model of the two passes against the float64 formula;
4. the function that chooses between the two kernel forms, at its bound and one beyond, and the real tile spans against the LDS
   array it guards;
5. header text, exports, ABI version;
6. the torch methods' new keyword, on CPU tensors;
7. the listing of the resample_aa_* kernels."""
import ctypes as C
import functools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd import torch_api
import resize_aa_reference as R

ROOT = Path(__file__).resolve().parent.parent
AXES = [(1, 1), (9, 4), (19, 1), (200, 13), (1080, 720), (11, 22)]


@pytest.fixture(scope="module")
def built():
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return S.load_library()


# ---- 1: the formula against torch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,sw,dh,dw", R.SHAPES, ids=lambda v: str(v))
def test_formula_against_torch_float64(sh, sw, dh, dw):
    x, ref = R.case(sh, sw, dh, dw)
    diff = np.abs(R.torch64(x, dh, dw) - ref).max()
    print(f"{sh}x{sw} -> {dh}x{dw}: max|torch float64 - formula| = {diff:.3g}")
    assert diff <= 1e-12 * float(np.abs(x).max())


# ---- 2: the library's table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,n", sorted({(sw, dw) for _, sw, _, dw in R.SHAPES} | {(sh, dh) for sh, _, dh, _ in R.SHAPES} | set(AXES)))
def test_table_equals_the_numpy_table_bit_for_bit(built, s, n):
    first, count, coef = S.cubic_aa_f32_taps(s, n)
    f32, c32, w32 = R.taps32(s, n)
    assert first.dtype == np.int32 and count.dtype == np.int32 and coef.dtype == np.float32
    assert np.array_equal(first, f32) and np.array_equal(count, c32)
    assert coef.shape == w32.shape and np.array_equal(coef.view(np.uint32), w32.view(np.uint32))


@pytest.mark.parametrize("s,n", AXES)
def test_table_invariants(built, s, n):
    first, count, coef = S.cubic_aa_f32_taps(s, n)
    assert (count >= 1).all() and (first >= 0).all() and (first + count <= s).all()
    assert coef.shape == (n, int(count.max())), "the returned maximum is the real one"
    assert built.srcnn_cubic_aa_f32_taps(s, n, None, None, None, 0) == int(count.max())
    pad = np.arange(coef.shape[1])[None, :] >= count[:, None]
    assert (coef[pad] == 0).all() and np.abs(coef.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -21
    # a wider table than needed: the same rows, more padding
    ip = C.POINTER(C.c_int)
    wide = np.full((n, coef.shape[1] + 3), np.float32(7))
    f2, c2 = np.empty(n, np.int32), np.empty(n, np.int32)
    assert built.srcnn_cubic_aa_f32_taps(s, n, f2.ctypes.data_as(ip), c2.ctypes.data_as(ip), S._fp(wide), wide.shape[1]) == coef.shape[1]
    assert np.array_equal(f2, first) and np.array_equal(c2, count)
    assert np.array_equal(wide[:, :coef.shape[1]], coef) and (wide[:, coef.shape[1]:] == 0).all()


@pytest.mark.parametrize("n", [1, 7, 64])
def test_the_same_size_holds_exactly_one_1(built, n):
    first, count, coef = S.cubic_aa_f32_taps(n, n)
    assert ((coef == 1.0).sum(axis=1) == 1).all() and ((coef != 0).sum(axis=1) == 1).all()
    assert np.array_equal(first + np.argmax(coef, axis=1), np.arange(n)), "and it sits on the sample itself"


def test_table_query_form_and_refusals(built):
    ip = C.POINTER(C.c_int)
    first, count, coef = np.empty(4, np.int32), np.empty(4, np.int32), np.empty((4, 16), np.float32)
    fp, cp, wp = first.ctypes.data_as(ip), count.ctypes.data_as(ip), S._fp(coef)
    taps = built.srcnn_cubic_aa_f32_taps
    assert taps(9, 4, None, None, None, 0) == 8 and taps(9, 4, fp, cp, None, 0) == 8          # the query writes nothing
    assert taps(9, 4, fp, cp, wp, 16) == 8
    for bad in ((0, 4, fp, cp, wp, 16), (9, -1, fp, cp, wp, 16), (0, 4, None, None, None, 0), (9, 4, None, cp, wp, 16),
                (9, 4, fp, None, wp, 16), (9, 4, fp, cp, wp, 7), (9, 4, fp, cp, wp, 0)):
        assert taps(*bad) == S.ERR_INVALID, bad[:2] + bad[5:]
    with pytest.raises(ValueError):
        S.cubic_aa_f32_taps(0, 3)
    assert built.srcnn_abi_version() == 1


# ---- 3: the float32 model against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,sw,dh,dw", R.SHAPES, ids=lambda v: str(v))
def test_float32_model_against_the_formula(sh, sw, dh, dw):
    x, ref = R.case(sh, sw, dh, dw)
    got = R.model32(x, R.taps32(sw, dw), R.taps32(sh, dh))
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"{sh}x{sw} -> {dh}x{dw}: max|model32 - formula| = {err:.3g}")
    assert err <= R.TOL * float(np.abs(x).max())


def test_model_properties():
    x = R.uniform((5, 7), 3)
    assert np.array_equal(R.model32(x, R.taps32(7, 7), R.taps32(5, 5)), x)                    # the same size: value for value
    const = R.model32(np.full((40, 50), np.float32(0.3)), R.taps32(50, 17), R.taps32(40, 9))
    assert np.abs(const.astype(np.float64) - np.float64(np.float32(0.3))).max() <= R.TOL * 0.3
    # antialiasing: the finest checkerboard, halved, is flat (4-tap sampling would keep it)
    board = (np.indices((32, 32)).sum(axis=0) % 2).astype(np.float32)
    assert np.abs(R.ref64(board, 16, 16)[4:-4, 4:-4] - 0.5).max() < 1e-3


# ---- 4: the form-choosing function -----------------------------------------------------------------------------------------
_tuning = None


def tuning_lib():
    global _tuning
    if _tuning is None:
        B.build()
        _tuning = C.CDLL(str(S.tuning_library_path()))
        _tuning.srcnn_debug_resample_aa_variant.argtypes = [C.c_int] * 4
        _tuning.srcnn_debug_resample_aa_limits.argtypes = [C.POINTER(C.c_int)]
    return _tuning


def limits():
    out = (C.c_int * 5)()
    assert tuning_lib().srcnn_debug_resample_aa_limits(out) == 0
    return dict(zip(("TR", "TC", "RATIO", "KMAX", "RMAX"), out))


def test_limits_hook_reports_the_documented_geometry():
    assert limits() == {"TR": 16, "TC": 64, "RATIO": 4, "KMAX": 17, "RMAX": 80}


def test_form_choice_at_its_bound_and_one_beyond():
    variant = tuning_lib().srcnn_debug_resample_aa_variant          # (sw, sh, dw, dh) -> 1 tiled, 0 general
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)):
        assert variant(*bad) < 0
    for dw, dh in ((64, 16), (65, 17), (100, 30), (480, 270)):
        assert variant(4 * dw, 4 * dh, dw, dh) == 1, "ratio 4 on both axes: tiled"
        assert variant(4 * dw + 1, 4 * dh, dw, dh) == 0, "one column beyond"
        assert variant(4 * dw, 4 * dh + 1, dw, dh) == 0, "one row beyond"
        assert variant(4 * dw + 1, dh, dw, dh) == 0 and variant(dw, 4 * dh + 1, dw, dh) == 0, "one axis inside, one outside: general"
        assert variant(dw, dh, dw, dh) == 1 and variant(dw, dh, 2 * dw, 2 * dh) == 1 and variant(3 * dw, 2 * dh, dw, dh) == 1
    assert variant(3840, 2160, 1920, 1080) == 1 and variant(3840, 2160, 2560, 1440) == 1 and variant(131, 67, 87, 45) == 1
    assert variant(200, 3, 13, 2) == 0 and variant(19, 17, 1, 1) == 0 and variant(3840, 2160, 160, 90) == 0


def test_selected_tiles_fit_the_lds_array(built):
    """hbuf[AA_RMAX][AA_TC] is indexed by the rows a tile REALLY spans, taken here from the product's own table; the
    form-choosing function is the only guard.  The axes are independent in the choice, so the row axis is swept against a column
    axis that always qualifies (1 -> 1).  Also what the kernels rest on: first and first + count never decrease."""
    lim, variant = limits(), tuning_lib().srcnn_debug_resample_aa_variant
    worst, kmax, tiled = 0, 0, 0
    for n in list(range(1, 70)) + [100, 127, 333, 1080]:
        for s in sorted(set(list(range(1, 4 * n + 3))[::max(1, n // 8)] + [n, 2 * n, 3 * n, 4 * n - 1, 4 * n, 4 * n + 1])):
            first, count, _ = S.cubic_aa_f32_taps(s, n)
            assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()
            if variant(1, s, 1, n) == 1:
                tiled += 1
                lo = np.arange(0, n, lim["TR"])
                hi = np.minimum(lo + lim["TR"] - 1, n - 1)
                worst = max(worst, int((first[hi] + count[hi] - first[lo]).max()))
                kmax = max(kmax, int(count.max()))
            else:
                assert s > lim["RATIO"] * n or count.max() > lim["KMAX"]
    print(f"largest real row span among {tiled} tiled axes: {worst} (capacity {lim['RMAX']}), most taps {kmax} (capacity {lim['KMAX']})")
    assert tiled > 1000 and worst <= lim["RMAX"] and kmax <= lim["KMAX"]


# ---- 5: header, exports, ABI -----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["srcnn_cubic_aa_f32_taps", "srcnn_resize_cubic_aa_f32", "srcnn_resize_cubic_aa_f32_dev", "srcnn_resize_cubic_aa_image_dev"]


def test_header_exports_and_abi(built):
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    for needle in ("antialias=True", "A = -0.5", "xmin = max(0, trunc((c - support) + 0.5))", "w_j = w_j / total", "only finite input is tested",
                   "Matlab's imresize pads its borders", "zero for j >= count[d]"):
        assert needle in text, needle
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in exported and name in S.ABI_SYMBOLS and hasattr(built, name), name
    assert not any("resample_aa" in n for n in exported), "the hooks and the launchers stay out of the product"
    assert built.srcnn_abi_version() == 1
    assert "down-scaling is plain 4-tap sampling without antialiasing" in text, "the existing resize's text is unchanged"


# ---- 6: the torch methods on CPU tensors -----------------------------------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


def test_torch_methods_take_the_keyword_and_refuse_before_the_library():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 3, 0, None
    x, u8 = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(ValueError, match="antialias"):
            fast.resize(x, (4, 4), antialias=bad)
        with pytest.raises(ValueError, match="antialias"):
            fast.resize_image(u8, (4, 4), antialias=bad)
    # the keyword is accepted, and the existing refusals and their messages are what they were, with it and without
    for aa in (False, True):
        with pytest.raises(ValueError, match=r"expected a tensor on cuda:0, got one on cpu \(there is no CPU path\)"):
            fast.resize(x, (4, 4), antialias=aa)
        with pytest.raises(ValueError, match=r"expected a tensor on cuda:0, got one on cpu \(there is no CPU path\)"):
            fast.resize_image(u8, (4, 4), antialias=aa)
        with pytest.raises(ValueError, match="expected a float32 tensor"):
            fast.resize(x.double(), (4, 4), antialias=aa)
        with pytest.raises(ValueError, match="expected two positive integers"):
            fast.resize_image(u8, (0, 4), antialias=aa)
        with pytest.raises(ValueError, match="in_scale"):
            fast.resize_image(u8, (4, 4), in_scale=0.0, antialias=aa)
    with pytest.raises(ValueError, match="there is no CPU path"):
        fast.resize(x, (4, 4))
    import inspect
    for name in ("upscale", "upscale_rgb", "upscale_image", "upscale_rgb_image", "forward_image"):
        assert "antialias" not in inspect.signature(getattr(torch_api.CompiledModule, name)).parameters, name


def test_python_binding_refuses_before_the_library():
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = _NoCall(), None
    good = np.zeros((3, 8, 8), np.float32)
    with pytest.raises(TypeError):
        ctx.resize_cubic_aa_f32(good.astype(np.float64), 4, 4)
    with pytest.raises(ValueError):
        ctx.resize_cubic_aa_f32(np.zeros((3, 8, 16), np.float32)[:, :, ::2], 4, 4)
    for bad in ((0, 4), (4, -1), (4.0, 4), (True, 4)):
        with pytest.raises(ValueError):
            ctx.resize_cubic_aa_f32(good, *bad)


# ---- 7: the listing --------------------------------------------------------------------------------------------------------
UNIT = "srcnn_pipeline.hip"
AA_KERNELS = {"resample_aa_tiled_kernel": 4 * 80 * 64, "resample_aa_h_kernel": 0, "resample_aa_v_kernel": 0}
OLD_SUBSTRINGS = ["resize_cubic_image_tiled_kernel", "resize_cubic_image_direct_kernel", "luma_resize_image_kernel", "luma_resize_f32_kernel",
                  "resize_merge_f32_kernel", "resize_cubic_f32_tiled_kernel", "resize_merge_image_kernel", "resize_merge_image_pixels_kernel",
                  "convert_image_kernelILi1E", "convert_image_kernelILi3E"]


@functools.lru_cache(maxsize=None)
def pipeline_listing():
    flags = [u[1] for u in B.UNITS if u[0] == UNIT and len(u) == 2][0]
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "unit.s"
        subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, f"-I{B.CSRC}", "-S", "--cuda-device-only",
                        "-o", str(out), str(B.CSRC / UNIT)], check=True, stderr=subprocess.DEVNULL)
        text = out.read_text()
    return dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)), text


def test_the_listing_holds_exactly_the_three_kernels():
    descs, _ = pipeline_listing()
    assert sorted(n for n in descs if "resample_aa_" in n) == sorted(n for n in descs if any(k in n for k in AA_KERNELS))
    assert sum("resample_aa_" in n for n in descs) == len(AA_KERNELS)
    for old in OLD_SUBSTRINGS:
        assert sum(old in n for n in descs) == 1, old


@pytest.mark.parametrize("kernel", sorted(AA_KERNELS))
def test_resample_kernels_use_no_scratch_no_contraction_and_the_stated_lds(kernel):
    descs, text = pipeline_listing()
    mine = [n for n in descs if kernel in n]
    assert len(mine) == 1, mine
    field = lambda f: int(re.search(rf"\.amdhsa_{f} (\d+)", descs[mine[0]]).group(1))
    assert field("private_segment_fixed_size") == 0
    meta = re.search(rf"\.name:\s+{re.escape(mine[0])}\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert meta and int(meta.group(1)) == 0
    assert field("group_segment_fixed_size") == AA_KERNELS[kernel], "DESIGN.md 4.15 states the tile's LDS"
    body = re.search(rf"^{re.escape(mine[0])}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M).group(1)
    assert "v_mul_f32" in body and "v_add_f32" in body
    assert not re.search(r"\bv_(fma|fmac|mad|mac)_f32\b", body), "no contraction: every product and sum is rounded on its own"
    design = (ROOT / "DESIGN.md").read_text()
    assert "4.15" in design and (AA_KERNELS[kernel] == 0 or f"{AA_KERNELS[kernel]:,} bytes" in design)
