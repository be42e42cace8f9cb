"""CPU tests of the full-reference metrics (srcnn_metrics_image_dev, srcnn_metric_psnr): no device.
1. the numpy statement (tests/metrics_reference.py) against a direct, non-separable evaluation of the definition, its closed
   forms, and the float32 cancellation the float64 arithmetic is there to avoid;
2. header text, exports, ABI version, srcnn_metric_psnr;
3. the torch methods and the Python binding refuse bad arguments on CPU tensors, before the library is reached;
4. the listing of the metric_* kernels."""
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

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd import torch_api
import metrics_reference as R

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def built():
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return S.load_library()


# ---- 1: the reference ------------------------------------------------------------------------------------------------------
def test_window_is_the_stated_gaussian():
    g = R.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) <= 2e-16 and np.array_equal(g, g[::-1])
    assert abs(g[5] / g[4] - math.exp(1 / 4.5)) <= 1e-15


@pytest.mark.parametrize("L", [1.0, 255.0])
def test_separable_reference_against_the_direct_definition(L):
    a, b = R.load(R.noise((13, 14), 1, L)), R.load(R.smooth((13, 14), 2, L))
    diff = np.abs(R.ssim_map(a, b, L) - R.ssim_map_direct(a, b, L)).max()
    print(f"13 x 14, L = {L}: max|separable - direct| = {diff:.3g}")
    assert R.ssim_map(a, b, L).shape == (3, 4) and diff <= 1e-13


@pytest.mark.parametrize("L,c,d", [(1.0, 0.25, 0.125), (255.0, 100.0, -3.0), (1.0, 0.5, 0.0)])
def test_closed_form_on_constant_planes(L, c, d):
    a, b = np.full((1, 20, 23), c), np.full((1, 20, 23), c + d)
    m = R.metrics(a, b, border=2, data_range=L)[0]
    n = 16 * 19
    c1 = (0.01 * L) ** 2
    assert m[1] == n and m[3] == 6 * 9
    assert abs(m[0] - n * d * d) <= 1e-12 * max(1.0, n * d * d)
    assert abs(m[2] / m[3] - (2 * c * (c + d) + c1) / (c * c + (c + d) ** 2 + c1)) <= 1e-12


def test_identical_planes_give_exactly_one():
    for x in (R.load(R.noise((3, 17, 19), 3)), R.load(R.smooth((3, 17, 19), 4, 255.0)), R.load(R.near_constant((3, 17, 19))[1])):
        for luma in (None, R.LUMA_BT601):
            m = R.metrics(x, x.copy(), luma=luma, data_range=1.0)
            assert (m[:, 0] == 0).all() and np.array_equal(m[:, 2], m[:, 3]) and m[0, 3] == 7 * 9
            ya = x if luma is None else R.luma_of(x, luma)[None]
            assert (R.ssim_map(ya[0], ya[0], 1.0) == 1.0).all()


def test_unselected_metric_fields_are_zero_and_luma_is_one_result():
    a, b = R.load(R.noise((3, 12, 12), 5)), R.load(R.noise((3, 12, 12), 6))
    assert R.metrics(a, b, luma=R.LUMA_BT601).shape == (1, 4) and R.metrics(a, b).shape == (3, 4)
    assert (R.metrics(a, b, ssim=False)[:, 2:] == 0).all() and (R.metrics(a, b, sse=False)[:, :2] == 0).all()


@pytest.mark.parametrize("L", [1.0, 255.0])
def test_float32_cancels_where_float64_does_not(L):
    """The case the float64 arithmetic is for: a plane at 0.999 L, one pixel changed.  The same formula in float32 is off by
    more than 1e-5 on some window; the float64 statement agrees with the direct evaluation within 1e-10, the level at which
    float64 itself cancels here: a few dozen roundings of 2^-53 on E[x^2] ~ L^2 against C2 = 9e-4 L^2."""
    a32, b32 = R.near_constant((24, 24), L)
    a, b = R.load(a32), R.load(b32)
    ref = R.ssim_map(a, b, L)
    assert np.abs(ref - R.ssim_map_direct(a, b, L)).max() <= 1e-10
    g = R.window().astype(np.float32)
    blur32 = lambda p: R._valid(R._valid(p, g, 0), g, 1)
    c1, c2 = np.float32((0.01 * L) ** 2), np.float32((0.03 * L) ** 2)
    ma, mb, eaa, ebb, eab = blur32(a32), blur32(b32), blur32(a32 * a32), blur32(b32 * b32), blur32(a32 * b32)
    m32 = ((2 * ma * mb + c1) * (2 * (eab - ma * mb) + c2)) / ((ma * ma + mb * mb + c1) * ((eaa - ma * ma) + (ebb - mb * mb) + c2))
    assert m32.dtype == np.float32
    worst = np.abs(m32.astype(np.float64) - ref).max()
    print(f"L = {L}: a float32 model of the formula is off by {worst:.3g} on its worst window")
    assert worst > 1e-5


@pytest.mark.parametrize("luma,border,shape", [(None, 0, (22, 3, 12, 13)), (R.LUMA_BT601, 1, (64, 3, 14, 15)), (None, 0, (64, 1, 3, 5))])
def test_batched_reference_equals_the_loop_form(luma, border, shape):
    """metrics_batch (all planes at once, for the tests that measure 65,538 planes) against metrics() frame by frame, on 64
    planes or more: the counts to the last bit, the sums within 1e-15 relative."""
    a, b = R.load(R.noise(shape, 21)), R.load(R.smooth(shape, 22))
    ssim = shape[-1] - 2 * border >= R.WIN
    got = R.metrics_batch(a, b, border=border, luma=luma, ssim=ssim)
    want = np.stack([R.metrics(a[f], b[f], border=border, luma=luma, ssim=ssim) for f in range(shape[0])])
    assert got.shape == want.shape and got.shape[0] * got.shape[1] >= 64
    assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 3], want[..., 3])
    for k in (0, 2):
        assert (np.abs(got[..., k] - want[..., k]) <= 1e-15 * np.abs(want[..., k])).all()
    assert (want[..., 0] > 0).all() and ((want[..., 2] != 0).all() or not ssim)


def test_ssim_of_a_row_periodic_picture_is_the_sum_of_its_bands():
    """The identity the GPU test of the SSIM band walk rests on, here on 5 bands and the window row that closes the picture: a
    pair whose rows repeat with the band height B = 64 gives every full band the same 74 source rows, so
    ssim_sum = 5 S(74 x 11) + S(11 x 11).  Both sides are float64 sums of the same window values; they differ by the rounding
    of one sum against five."""
    B, W, k = 64, 11, 5
    rng = np.random.default_rng(31)
    blocks = [rng.integers(0, 256, (B, W), dtype=np.uint8) for _ in range(2)]
    rows = k * B + R.WIN
    a, b = (R.load(R.periodic_rows(x, rows))[None] for x in blocks)
    whole = R.metrics(a, b, sse=False)[0]
    band = R.metrics(a[:, :B + R.WIN - 1], b[:, :B + R.WIN - 1], sse=False)[0]
    last = R.metrics(a[:, :R.WIN], b[:, :R.WIN], sse=False)[0]
    assert np.array_equal(a[0, k * B:], a[0, :R.WIN]) and band[3] == B and last[3] == 1
    assert whole[3] == k * band[3] + last[3] == rows - R.WIN + 1
    want = math.fsum([band[2]] * k + [last[2]])
    assert abs(whole[2] - want) <= 1e-14 * max(abs(want), abs(band[2])), "three correctly rounded sums: a few 2^-53 apart"
    assert abs(whole[2] / whole[3]) < 0.5, "two unrelated pictures"


# ---- 2: header, exports, ABI, psnr -----------------------------------------------------------------------------------------
NEW_SYMBOLS = ["srcnn_metrics_image_dev", "srcnn_metric_psnr"]


def test_header_exports_and_abi(built):
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    for needle in ("EVERYTHING AFTER THE LOAD IS FLOAT64", "y = ((w0 c0 + w1 c1) + w2 c2) + offset", "g[i] = exp(-(i - 5)^2 / 4.5)",
                   "C1 = (0.01 L)^2, C2 = (0.03 L)^2", "{sse, n_px, ssim_sum, n_win}", "no floating-point atomic", "MS-SSIM",
                   "rgb2ycbcr", "returning an SSIM map", "SRCNN_METRIC_SSE = 1, SRCNN_METRIC_SSIM = 2"):
        assert needle in text, needle
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in exported and name in S.ABI_SYMBOLS and hasattr(built, name), name
    assert not any("launch_metrics" in n or "debug_metric" in n for n in exported), "the hook and the launcher stay out of the product"
    assert built.srcnn_abi_version() == 1
    assert (S.METRIC_SSE, S.METRIC_SSIM) == (1, 2) and S.METRIC_FIELDS == ("sse", "n_px", "ssim_sum", "n_win")


def test_metric_psnr_values(built):
    assert S.metric_psnr(0.0, 100.0, 1.0) == math.inf
    assert S.metric_psnr(1.0, 100.0, 1.0) == pytest.approx(20.0, abs=1e-12)
    assert S.metric_psnr(100.0, 100.0, 255.0) == pytest.approx(20.0 * math.log10(255.0), abs=1e-12)
    assert S.metric_psnr(2.5, 640.0 * 480.0, 1.0) == pytest.approx(10.0 * math.log10(640 * 480 / 2.5), abs=1e-12)
    for bad in ((-1.0, 10.0, 1.0), (1.0, 0.0, 1.0), (1.0, 10.0, 0.0), (math.nan, 10.0, 1.0), (1.0, 10.0, -2.0)):
        assert math.isnan(S.metric_psnr(*bad)), bad


def test_tuning_hook_reports_the_documented_tile():
    B.build()
    lib = C.CDLL(str(S.tuning_library_path()))
    out = (C.c_int * 4)()
    assert lib.srcnn_debug_metric_limits(out) == 0 and lib.srcnn_debug_metric_limits(None) == S.ERR_INVALID
    assert list(out) == [54, 64, 4, 2560]


# ---- 3: refusals before the library ----------------------------------------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


def shell_module():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 1, 0, None
    return fast


def test_torch_methods_refuse_on_cpu_tensors_before_the_library():
    fast = shell_module()
    x3, x1 = torch.zeros(2, 3, 16, 16), torch.zeros(1, 16, 16)
    for method in (fast.metrics, fast.psnr, fast.ssim):
        with pytest.raises(ValueError, match="two torch.Tensors"):
            method(x3, np.zeros((2, 3, 16, 16), np.float32))
        with pytest.raises(ValueError, match="same shape"):
            method(x3, torch.zeros(2, 3, 16, 15))
        with pytest.raises(ValueError, match="same shape"):
            method(torch.zeros(16, 16), torch.zeros(16, 16))
        with pytest.raises(ValueError, match="1 or 3 channels"):
            method(torch.zeros(2, 16, 16), torch.zeros(2, 16, 16))
        with pytest.raises(ValueError, match="float32, float16, bfloat16 or uint8"):
            method(x3.double(), x3.double())
        with pytest.raises(ValueError, match="float32, float16, bfloat16 or uint8"):
            method(x3, x3.double())
        with pytest.raises(ValueError, match="must be positive"):
            method(x3, torch.zeros(2, 3, 16, 1).expand(2, 3, 16, 16))      # a stride of 0
        with pytest.raises(ValueError, match="in_scale"):
            method(x3.to(torch.uint8), x3, in_scale=0.0)
        for bad in (-1, 1.0, True, None):
            with pytest.raises(ValueError, match="border"):
                method(x3, x3, border=bad)
        with pytest.raises(ValueError, match="luma needs 3 channels"):
            method(x1, x1, luma=S.LUMA_BT601)
        for bad in ((1.0, 2.0, 3.0), (0.3, 0.6, math.nan, 0.0), (0.3, math.inf, 0.1, 0.0), "rgb"):
            with pytest.raises(ValueError, match="luma"):
                method(x3, x3, luma=bad)
        for bad in (0.0, -1.0, math.inf, math.nan, "wide"):
            with pytest.raises(ValueError, match="data_range"):
                method(x3, x3, data_range=bad)
        with pytest.raises(ValueError, match="leaves nothing"):
            method(x3, x3, border=8)
        # everything is in order but the device: there is no CPU path
        with pytest.raises(ValueError, match=r"expected a tensor on cuda:0, got one on cpu \(there is no CPU path\)"):
            method(x3, x3.to(torch.float16), border=2, luma=(0.0, 0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="ssim"):
        fast.metrics(x3, x3, ssim=1)
    for method in (fast.metrics, fast.ssim):
        with pytest.raises(ValueError, match="at least 11 x 11"):
            method(x3, x3, border=3)
    with pytest.raises(ValueError, match="there is no CPU path"):      # the squared error alone needs no window
        fast.psnr(x3, x3, border=3)
    with pytest.raises(ValueError, match="there is no CPU path"):
        fast.metrics(x3, x3, border=3, ssim=False)


def test_python_binding_refuses_a_bad_luma_before_the_library():
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = _NoCall(), None
    im = S.Image(256, S.ELEM_F32, 1, 16, 256, 768)
    for bad in ((1.0, 2.0), (math.nan, 0.0, 0.0, 0.0), "y"):
        with pytest.raises(ValueError, match="luma"):
            ctx.metrics_image_dev(im, im, 16, 16, 3, 1, 0, bad, 1.0, S.METRIC_SSE, 512)
    with pytest.raises(ValueError, match="must not be negative"):
        ctx.metrics_image_dev(S.Image(256, S.ELEM_F32, 1, -16), im, 16, 16, 1, 1, 0, None, 1.0, S.METRIC_SSE, 512)


# ---- 4: the listing --------------------------------------------------------------------------------------------------------
UNIT = "srcnn_metrics.hip"
METRIC_KERNELS = {"metric_sse_kernel": 256 * 8, "metric_ssim_kernel": 5 * 64 * 8, "metric_finish_kernel": 256 * 8}


@functools.lru_cache(maxsize=None)
def metrics_listing():
    flags = [u[1] for u in B.UNITS if u[0] == UNIT and len(u) == 2][0]
    assert "-ffp-contract=off" in flags
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "unit.s"
        subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, f"-I{B.CSRC}", "-S", "--cuda-device-only",
                        "-o", str(out), str(B.CSRC / UNIT)], check=True, stderr=subprocess.DEVNULL)
        text = out.read_text()
    return dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)), text


def test_the_listing_holds_exactly_the_three_kernels():
    descs, _ = metrics_listing()
    assert len(descs) == len(METRIC_KERNELS)
    for k in METRIC_KERNELS:
        assert sum(k in n for n in descs) == 1, k


@pytest.mark.parametrize("kernel", sorted(METRIC_KERNELS))
def test_metric_kernels_use_no_scratch_and_the_stated_lds(kernel):
    descs, text = metrics_listing()
    name = [n for n in descs if kernel in n][0]
    field = lambda f: int(re.search(rf"\.amdhsa_{f} (\d+)", descs[name]).group(1))
    assert field("private_segment_fixed_size") == 0
    meta = re.search(rf"\.name:\s+{re.escape(name)}\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert meta and int(meta.group(1)) == 0
    assert field("group_segment_fixed_size") == METRIC_KERNELS[kernel], "DESIGN.md 4.16 states the LDS"
    body = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M).group(1)
    assert "v_add_f64" in body and "atomic" not in body, "float64 sums, and no atomic of any kind"
    if kernel == "metric_ssim_kernel":
        assert "v_fma_f64" in body and "v_mul_f64" in body and ("ds_read" in body or "ds_load" in body)
    design = (ROOT / "DESIGN.md").read_text()
    assert "4.16" in design and f"{METRIC_KERNELS['metric_ssim_kernel']:,} bytes" in design
