"""CPU tests of MS-SSIM (srcnn_msssim_image_dev, srcnn_metric_msssim): no device.
1. the numpy statement (tests/msssim_reference.py) against a float64 torch script at an all-even size, against a direct,
   non-separable evaluation on its two smallest scales, its exact cases, and its reduction against an explicit padded copy;
2. srcnn_metric_msssim against numpy;
3. header text, exports, binding list, ABI version;
4. the torch methods and the Python binding refuse bad arguments on CPU tensors, before the library is reached;
5. the listing of the msssim_* kernels."""
import ctypes as C
import functools
import math
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd import torch_api
import metrics_reference as R
import msssim_reference as M

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def built():
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return S.load_library()


def noisy_pair(shape, seed, L=1.0, sigma=0.05):
    """the `smooth` picture and itself plus sigma L noise: mean cs per scale between 0.7 and 1, a product worth testing"""
    a = R.smooth(shape, seed, L)
    b = np.clip(a + sigma * L * np.random.default_rng(seed + 100).standard_normal(shape), 0.0, L).astype(np.float32)
    return R.load(a), R.load(b)


# ---- 1: the reference ------------------------------------------------------------------------------------------------------
def test_window_counts_and_scale_0_is_the_existing_ssim():
    a, b = noisy_pair((161, 161), 1)
    sums = M.msssim_plane(a, b, 1.0, 5)
    assert sums[:, 2].tolist() == [22801, 5041, 961, 121, 1]
    assert [p.shape for p in M.pyramid(a, 5)] == [(161, 161), (81, 81), (41, 41), (21, 21), (11, 11)]
    assert sums[0, 1] == R.ssim_plane(a, b, 1.0)[0], "scale 0's ssim_sum is metrics_reference.ssim_plane to the bit"
    assert M.msssim_plane(a, b, 1.0, 1)[0].tolist() == sums[0].tolist()
    assert [M.min_side(s) for s in (1, 2, 5)] == [11, 21, 161]


def torch_script(a, b, L, n_scales, dtype=torch.float64):
    """The usual script: conv2d with the 2-D window, avg_pool2d(2) between the scales -> (S, 2) mean cs, mean ssim"""
    a, b = (torch.from_numpy(x).to(dtype)[None, None] for x in (a, b))
    g = torch.from_numpy(R.window()).to(dtype)
    win = torch.outer(g, g)[None, None]
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    out = []
    for s in range(n_scales):
        blur = lambda t: F.conv2d(t, win)
        ma, mb, eaa, ebb, eab = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
        cs = (2 * (eab - ma * mb) + c2) / ((eaa - ma * ma) + (ebb - mb * mb) + c2)
        ssim = cs * (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
        out.append((float(cs.double().mean()), float(ssim.double().mean())))
        a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return np.array(out)


@pytest.mark.parametrize("L", [1.0, 255.0])
def test_statement_against_the_float64_torch_script_at_an_all_even_size(L):
    h, w = 176, 192                       # even at every one of the four reductions: avg_pool2d is the same reduction there
    assert h % 16 == 0 and w % 16 == 0
    a, b = noisy_pair((h, w), 2, L)
    sums = M.msssim_plane(a, b, L, 5)
    script = torch_script(a, b, L, 5)
    diff = np.abs(np.stack([sums[:, 0] / sums[:, 2], sums[:, 1] / sums[:, 2]], axis=1) - script).max()
    print(f"{h} x {w}, L = {L}: max|statement - torch float64 script| over the per-scale means = {diff:.3g}")
    assert diff <= 1e-12


def direct_maps(a, b, L):
    """cs and ssim window by window with the 2-D window g g^T: no separable pass"""
    g2 = np.outer(R.window(), R.window())
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    h, w = a.shape[0] - 10, a.shape[1] - 10
    cs, ssim = np.empty((h, w)), np.empty((h, w))
    for y in range(h):
        for x in range(w):
            pa, pb = a[y:y + R.WIN, x:x + R.WIN], b[y:y + R.WIN, x:x + R.WIN]
            ma, mb = (g2 * pa).sum(), (g2 * pb).sum()
            eaa, ebb, eab = (g2 * pa * pa).sum(), (g2 * pb * pb).sum(), (g2 * pa * pb).sum()
            cs[y, x] = (2 * (eab - ma * mb) + c2) / ((eaa - ma * ma) + (ebb - mb * mb) + c2)
            ssim[y, x] = cs[y, x] * (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
    return cs, ssim


@pytest.mark.parametrize("L", [1.0, 255.0])
def test_statement_against_the_direct_definition_on_the_two_smallest_scales(L):
    a, b = noisy_pair((161, 163), 3, L)
    sums = M.msssim_plane(a, b, L, 5)
    pa, pb = M.pyramid(a, 5), M.pyramid(b, 5)
    for s in (3, 4):
        cs, ssim = direct_maps(pa[s], pb[s], L)
        assert cs.size == sums[s, 2] and cs.shape == ((11, 11), (1, 1))[s - 3]
        diff = max(abs(cs.mean() - sums[s, 0] / sums[s, 2]), abs(ssim.mean() - sums[s, 1] / sums[s, 2]))
        print(f"scale {s}, L = {L}: |separable - direct| = {diff:.3g}")
        assert diff <= 1e-13


def test_identical_pictures_give_exactly_n_win_and_swapping_changes_nothing():
    x = R.load(R.smooth((3, 163, 171), 4, 255.0))
    for luma in (None, R.LUMA_BT601):
        same = M.msssim_sums(x, x.copy(), border=1, luma=luma, data_range=255.0)
        assert same.shape == ((1, 5, 3) if luma else (3, 5, 3))
        assert np.array_equal(same[..., 0], same[..., 2]) and np.array_equal(same[..., 1], same[..., 2])
    a, b = noisy_pair((1, 161, 170), 5)
    assert np.array_equal(M.msssim_sums(a, b), M.msssim_sums(b, a))
    assert M.msssim_value(M.msssim_sums(a, a)[0]) == 1.0


@pytest.mark.parametrize("h,w", [(7, 9), (8, 9), (7, 8), (1, 5), (2, 2)])
def test_reduction_on_odd_sizes_against_an_explicit_padded_copy(h, w):
    p = R.load(R.noise((h, w), h * w))
    padded = np.pad(p, ((0, h % 2), (0, w % 2)), mode="symmetric")      # the odd last row / column once more
    want = ((padded[0::2, 0::2] + padded[0::2, 1::2]) + (padded[1::2, 0::2] + padded[1::2, 1::2])) * 0.25
    got = M.reduce2(p)
    assert got.shape == (-(-h // 2), -(-w // 2)) and np.array_equal(got, want)
    if h % 2 == 0 and w % 2 == 0:
        pooled = F.avg_pool2d(torch.from_numpy(p)[None, None], 2)[0, 0].numpy()
        assert np.abs(pooled - got).max() <= 2e-16


# ---- 2: srcnn_metric_msssim ------------------------------------------------------------------------------------------------
def test_metric_msssim_against_numpy(built):
    a, b = noisy_pair((176, 192), 6)
    sums = M.msssim_plane(a, b, 1.0, 5)
    m = M.means(sums)
    print("mean cs per scale (ssim at the last):", np.array2string(m, precision=4))
    assert (m > 0.5).all() and (m < 1.0).all(), "a product worth testing"
    want = M.msssim_value(sums)
    assert 0.5 < want < 1.0
    assert abs(S.metric_msssim(sums) - want) <= 1e-14 * want, "NULL weights: the published five"
    assert abs(S.metric_msssim(sums, M.WEIGHTS) - want) <= 1e-14 * want
    for n in (1, 2, 3, 4):
        w = np.linspace(0.2, 1.0, n)
        want_n = M.msssim_value(sums[:n], w)
        assert abs(S.metric_msssim(sums[:n], w) - want_n) <= 1e-14 * want_n, n
    # the last scale contributes its ssim, the others their cs
    assert S.metric_msssim(sums[:1], [1.0]) == pytest.approx(sums[0, 1] / sums[0, 2], rel=1e-15)
    assert S.metric_msssim(sums[:2], [1.0, 0.0]) == pytest.approx(sums[0, 0] / sums[0, 2], rel=1e-15)
    assert S.MSSSIM_WEIGHTS == M.WEIGHTS and S.MSSSIM_FIELDS == ("cs_sum", "ssim_sum", "n_win") and S.MSSSIM_MAX_SCALES == 5


def test_metric_msssim_clamps_a_mean_that_is_not_positive_to_zero(built):
    sums = np.array([[90.0, 95.0, 100.0]] * 5)
    assert S.metric_msssim(sums) > 0.0
    for s, k in ((0, 0), (2, 0), (4, 1)):          # the field scale s contributes
        for v in (-3.0, 0.0, -0.0):
            bad = sums.copy()
            bad[s, k] = v
            assert S.metric_msssim(bad) == 0.0 and M.msssim_value(bad) == 0.0, (s, v)
    unused = sums.copy()
    unused[4, 0], unused[1, 1] = -50.0, -50.0      # the fields that do not enter the product
    assert S.metric_msssim(unused) == S.metric_msssim(sums)


def test_metric_msssim_nan_cases(built):
    lib = built
    dp = C.POINTER(C.c_double)
    sums = np.array([[90.0, 95.0, 100.0]] * 5)
    w = np.full(5, 0.2)
    ptr = lambda x: x.ctypes.data_as(dp)
    assert lib.srcnn_metric_msssim(ptr(sums), 5, ptr(w)) > 0.0
    assert math.isnan(lib.srcnn_metric_msssim(None, 5, ptr(w))), "null sums"
    for n in (0, -1, 6):
        assert math.isnan(lib.srcnn_metric_msssim(ptr(sums), n, ptr(w))), n
    for n in (1, 2, 3, 4):
        assert math.isnan(lib.srcnn_metric_msssim(ptr(sums), n, None)), "NULL weights need five scales"
        assert math.isnan(S.metric_msssim(sums[:n]))
    for s in range(5):
        for k in range(3):
            bad = sums.copy()
            bad[s, k] = math.nan
            assert math.isnan(S.metric_msssim(bad, w)), (s, k)
        for v in (0.0, -1.0):
            bad = sums.copy()
            bad[s, 2] = v
            assert math.isnan(S.metric_msssim(bad, w)), "n_win <= 0"
        bad_w = w.copy()
        bad_w[s] = math.nan
        assert math.isnan(S.metric_msssim(sums, bad_w))
    assert math.isnan(S.metric_msssim(np.zeros((6, 3)) + 1.0, np.full(6, 0.1)))
    with pytest.raises(ValueError, match="n_scales, 3"):
        S.metric_msssim(np.zeros((5, 4)))
    with pytest.raises(ValueError, match="weights for 5 scales"):
        S.metric_msssim(sums, [0.5, 0.5])


# ---- 3: header, exports, ABI -----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["srcnn_msssim_image_dev", "srcnn_metric_msssim"]


def test_header_exports_binding_and_abi(built):
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    for needle in ("AT SCALE 0 ONLY", "out(y, x) = ((p(2y, 2x) + p(2y, 2x+1)) + (p(2y+1, 2x) + p(2y+1, 2x+1))) * 0.25",
                   "cs   = (2 (E[ab] - mu_a mu_b) + C2) / (((E[a^2] - mu_a^2) + (E[b^2] - mu_b^2)) + C2)",
                   "{cs_sum, ssim_sum, n_win}", "h', w' >= 10 * 2^(S - 1) + 1", "(0.0448, 0.2856, 0.3001, 0.2363, 0.1333)",
                   "a power of a negative number is never formed", "No floating-point atomic".lower()):
        assert needle in text, needle
    assert "Out of scope: MS-SSIM" not in text and "Out of scope: the uniform-window SSIM" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in exported and name in S.ABI_SYMBOLS and hasattr(built, name), name
    assert not any("launch_msssim" in n or "msssim_launcher" in n or "debug_msssim" in n for n in exported), \
        "the hook and the launcher stay out of the product"
    assert built.srcnn_abi_version() == 1
    assert "srcnn_msssim.hip" not in B.HOST_UNITS and ("srcnn_msssim.hip", ["-ffp-contract=off"]) in B.UNITS


def test_tuning_hook_reports_the_documented_tile():
    B.build()
    lib = C.CDLL(str(S.tuning_library_path()))
    out = (C.c_int * 5)()
    assert lib.srcnn_debug_msssim_limits(out) == 0 and lib.srcnn_debug_msssim_limits(None) == S.ERR_INVALID
    assert list(out) == [54, 64, 16, 4, 2560]


# ---- 4: refusals before the library ----------------------------------------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


def shell_module():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 1, 0, None
    return fast


def test_torch_methods_refuse_on_cpu_tensors_before_the_library():
    fast = shell_module()
    x3, x1 = torch.zeros(2, 3, 170, 165), torch.zeros(1, 170, 165)
    for method in (fast.msssim_sums, fast.msssim):
        with pytest.raises(ValueError, match="two torch.Tensors"):
            method(x3, np.zeros((2, 3, 170, 165), np.float32))
        with pytest.raises(ValueError, match="same shape"):
            method(x3, torch.zeros(2, 3, 170, 164))
        with pytest.raises(ValueError, match="1 or 3 channels"):
            method(torch.zeros(2, 170, 165), torch.zeros(2, 170, 165))
        with pytest.raises(ValueError, match="float32, float16, bfloat16 or uint8"):
            method(x3, x3.double())
        with pytest.raises(ValueError, match="must be positive"):
            method(x3, torch.zeros(2, 3, 170, 1).expand(2, 3, 170, 165))      # a stride of 0
        with pytest.raises(ValueError, match="in_scale"):
            method(x3.to(torch.uint8), x3, in_scale=0.0)
        for bad in (-1, 1.0, True, None):
            with pytest.raises(ValueError, match="border"):
                method(x3, x3, border=bad)
        with pytest.raises(ValueError, match="luma needs 3 channels"):
            method(x1, x1, luma=S.LUMA_BT601)
        for bad in ((1.0, 2.0, 3.0), (0.3, 0.6, math.nan, 0.0), "rgb"):
            with pytest.raises(ValueError, match="luma"):
                method(x3, x3, luma=bad)
        for bad in (0.0, -1.0, math.inf, math.nan, "wide"):
            with pytest.raises(ValueError, match="data_range"):
                method(x3, x3, data_range=bad)
        with pytest.raises(ValueError, match="leaves nothing"):
            method(x3, x3, border=83)
        w = {} if method == fast.msssim_sums else {"weights": (0.5,) * 6}
        for bad in (0, 6, 2.0, True, None):
            with pytest.raises(ValueError, match="n_scales|weights"):
                method(x3, x3, n_scales=bad, **w)
        # the size rule: 161 for five scales, 21 for two -- the message names S and the minimum
        with pytest.raises(ValueError, match="5 scales need a region of at least 161 x 161, this one is 164 x 159"):
            method(x3, x3, border=3)
        with pytest.raises(ValueError, match="5 scales need a region of at least 161 x 161, this one is 160 x 155"):
            method(x3, x3, border=5)
        two = {"n_scales": 2} if method == fast.msssim_sums else {"n_scales": 2, "weights": (0.5, 0.5)}
        with pytest.raises(ValueError, match="2 scales need a region of at least 21 x 21, this one is 20 x 21"):
            method(torch.zeros(1, 20, 21), torch.zeros(1, 20, 21), **two)
        # everything is in order but the device: there is no CPU path
        with pytest.raises(ValueError, match=r"expected a tensor on cuda:0, got one on cpu \(there is no CPU path\)"):
            method(x3, x3.to(torch.float16), border=2, luma=(0.0, 0.0, 0.0, 0.0))      # 166 x 161: five scales fit
        with pytest.raises(ValueError, match="there is no CPU path"):
            method(x3, x3, border=40, **two)
    for bad, n in (((0.5, 0.5), 5), ((0.2,) * 4 + (math.nan,), 5), ("abcde", 5), (None, 3)):
        with pytest.raises(ValueError, match="weights"):
            fast.msssim(x3, x3, n_scales=n, weights=bad)


def test_python_binding_refuses_a_bad_luma_before_the_library():
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = _NoCall(), None
    im = S.Image(256, S.ELEM_F32, 1, 200, 40000, 120000)
    for bad in ((1.0, 2.0), (math.nan, 0.0, 0.0, 0.0), "y"):
        with pytest.raises(ValueError, match="luma"):
            ctx.msssim_image_dev(im, im, 200, 200, 3, 1, 0, bad, 1.0, 5, 512)
    with pytest.raises(ValueError, match="must not be negative"):
        ctx.msssim_image_dev(S.Image(256, S.ELEM_F32, 1, -200), im, 200, 200, 1, 1, 0, None, 1.0, 5, 512)


# ---- 5: the listing --------------------------------------------------------------------------------------------------------
UNIT = "srcnn_msssim.hip"
MSSSIM_KERNELS = {"msssim_pyramid_kernel": 0, "msssim_window_kernel": 5 * 64 * 8, "msssim_finish_kernel": 256 * 8}


@functools.lru_cache(maxsize=None)
def msssim_listing():
    flags = [u[1] for u in B.UNITS if u[0] == UNIT and len(u) == 2][0]
    assert "-ffp-contract=off" in flags
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "unit.s"
        subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, f"-I{B.CSRC}", "-S", "--cuda-device-only",
                        "-o", str(out), str(B.CSRC / UNIT)], check=True, stderr=subprocess.DEVNULL)
        text = out.read_text()
    return dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)), text


def test_the_listing_holds_exactly_the_three_kernels():
    descs, _ = msssim_listing()
    assert len(descs) == len(MSSSIM_KERNELS)
    for k in MSSSIM_KERNELS:
        assert sum(k in n for n in descs) == 1, k


@pytest.mark.parametrize("kernel", sorted(MSSSIM_KERNELS))
def test_msssim_kernels_use_no_private_segment_and_the_stated_lds(kernel):
    descs, text = msssim_listing()
    name = [n for n in descs if kernel in n][0]
    field = lambda f: int(re.search(rf"\.amdhsa_{f} (\d+)", descs[name]).group(1))
    assert field("private_segment_fixed_size") == 0
    meta = re.search(rf"\.name:\s+{re.escape(name)}\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert meta and int(meta.group(1)) == 0
    assert field("group_segment_fixed_size") == MSSSIM_KERNELS[kernel], "DESIGN.md 4.20 states the LDS"
    design = (ROOT / "DESIGN.md").read_text()
    assert "4.20" in design and f"{MSSSIM_KERNELS['msssim_window_kernel']:,} bytes" in design
