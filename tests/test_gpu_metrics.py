"""The full-reference metrics on the GPU (srcnn_metrics_image_dev, CompiledModule.metrics / psnr / ssim) against the numpy
float64 statement of tests/metrics_reference.py.  All planes are small.

Tolerances (the issue's, with their derivation):
  SSE   a float64 sum of n non-negative terms, each exact to 2 roundings: relative error <= (n + 4) 2^-53 in any order; the
        reference adds the same terms exactly (math.fsum), so the bound holds against it.
  SSIM  each factor of a window carries a few dozen roundings of 2^-53 on quantities <= 2 L^2 against C1 = 1e-4 L^2, <~ 1e-10
        relative: |ssim_sum / n_win - reference| <= 1e-9 for data in [0, L]."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import srcnn_cpp_amd as S
from srcnn_cpp_amd.torch_api import compile_module, describe_image
import metrics_reference as R
from test_gpu_resize_f32 import make_module

pytestmark = pytest.mark.gpu

BOTH = S.METRIC_SSE | S.METRIC_SSIM
GUARD = 4          # doubles either side of d_out


@functools.lru_cache(maxsize=None)
def tile():
    """(T, B): window columns and window rows of one SSIM workgroup, from the tuning library's hook"""
    lib = C.CDLL(str(S.tuning_library_path()))
    out = (C.c_int * 4)()
    assert lib.srcnn_debug_metric_limits(out) == 0
    return out[0], out[1]


@pytest.fixture(scope="module")
def mctx():
    ctx = S.Context(0)          # no model: the metrics need none
    yield ctx
    ctx.close()


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def loaded(t, in_scale=None):
    """What the library loads from a tensor (N, C, H, W), as float64 numpy"""
    if t.dtype == torch.uint8:
        return R.load(t.cpu().numpy(), in_scale)
    return t.float().cpu().numpy().astype(np.float64)      # float16 and bfloat16 widen exactly


def measure(ctx, a, b, border=0, luma=None, L=1.0, flags=BOTH, in_scale=None):
    """srcnn_metrics_image_dev on two CUDA tensors (N, C, H, W) as they lie -> (N, P, 4) float64 numpy; the output sits between
    guards, which must come back untouched"""
    n, c, h, w = a.shape
    ia, ib = describe_image(a, c, in_scale)[0], describe_image(b, c, in_scale)[0]
    per_frame = 1 if luma is not None else c
    out = torch.full((n * per_frame * 4 + 2 * GUARD,), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.metrics_image_dev(ia, ib, w, h, c, n, border, luma, L, flags, out.data_ptr() + 8 * GUARD)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == -7.25).all() and (got[-GUARD:] == -7.25).all(), "d_out is written inside its bounds only"
    return got[GUARD:-GUARD].reshape(n, per_frame, 4)


def reference(a, b, border=0, luma=None, L=1.0, in_scale=None, **kw):
    la, lb = loaded(a, in_scale), loaded(b, in_scale)
    return np.stack([R.metrics(la[f], lb[f], border=border, luma=luma, data_range=L, **kw) for f in range(la.shape[0])])


def check(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got[..., 1], ref[..., 1]) and np.array_equal(got[..., 3], ref[..., 3]), "n_px and n_win"
    sse_err = np.abs(got[..., 0] - ref[..., 0]) / np.where(ref[..., 0] > 0, ref[..., 0], 1.0)
    bound = R.sse_bound(ref[..., 1])
    worst_ssim = 0.0
    if (ref[..., 3] > 0).any():
        worst_ssim = float(np.abs(got[..., 2] / got[..., 3] - ref[..., 2] / ref[..., 3]).max())
    print(f"{what}: SSE relative error {sse_err.max():.3g} (bound {bound.max():.3g}), |mean SSIM - reference| {worst_ssim:.3g}")
    assert (sse_err <= bound).all()
    assert worst_ssim <= R.SSIM_TOL
    return worst_ssim


def pair(shape, seed, L=1.0):
    return cuda(R.noise(shape, seed, L)), cuda(R.smooth(shape, seed + 1, L))


# ---- shapes ----------------------------------------------------------------------------------------------------------------
def region(name):
    """(h', w') of a named case: sizes that sit on the SSIM tile's column count T and band height B, one below and one above"""
    T, B = tile()
    fixed = {"one-window": (11, 11), "12x75": (12, 75)}
    if name in fixed:
        return fixed[name]
    kind, expr = name.split("=")
    n = eval(expr, {"T": T, "B": B})
    return (13, n + 10) if kind == "cols" else (n + 10, 23)


SHAPES = ["one-window", "12x75", "cols=T-1", "cols=T", "cols=T+1", "cols=2*T+1", "rows=B-1", "rows=B", "rows=B+1", "rows=2*B+1"]


@pytest.mark.parametrize("border", [0, 1, 4])
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_on_the_tile_bounds(mctx, name, border):
    rh, rw = region(name)
    a, b = pair((1, 1, rh + 2 * border, rw + 2 * border), rh + rw)
    got = measure(mctx, a, b, border=border)
    assert got[0, 0, 1] == rh * rw and got[0, 0, 3] == (rh - 10) * (rw - 10)
    check(got, reference(a, b, border=border), f"{name} ({rh} x {rw}), border {border}")


def test_the_hook_reports_a_tile_the_shapes_cross():
    T, B = tile()
    assert 1 < T <= 64 and B > 1
    assert region("cols=T+1") == (13, T + 11) and region("rows=2*B+1") == (2 * B + 11, 23)


def test_squared_error_alone_on_regions_too_small_for_a_window(mctx):
    for h, w, border in ((1, 1, 0), (3, 700, 0), (12, 9, 1), (300, 2, 0)):
        a, b = pair((2, 1, h, w), h * w)
        got = measure(mctx, a, b, border=border, flags=S.METRIC_SSE)
        check(got, reference(a, b, border=border, ssim=False), f"{h} x {w}, border {border}, SSE only")


# ---- the loops inside a workgroup and in the finish: regions past 1,024 columns and past 256 partials -------------------------
SSE_COLS = 4 * 256          # the columns one pass of the SSE kernel's 256 threads covers


@pytest.mark.parametrize("form", ["planar-f32", "interleaved-u8", "luma"])
@pytest.mark.parametrize("rh,rw", [(4, SSE_COLS + 1), (4, 2 * SSE_COLS + 1), (5, 2 * SSE_COLS + 3)], ids=lambda v: str(v))
def test_sse_column_groups_beyond_the_first(mctx, rh, rw, form):
    """A thread's second and third column group (x += 1024).  planar-f32 is the 16-byte form: 1025 and 2049 columns leave its last
    group one column wide (the scalar tail at x + 3 >= rw), 2051 three; 5 rows leave the second workgroup one row."""
    assert rw > SSE_COLS and rw % 4 != 0
    if form == "interleaved-u8":
        rng = np.random.default_rng(rw)
        a, b = (torch.from_numpy(rng.integers(0, 256, (2, rh, rw, 3), dtype=np.uint8)).cuda().permute(0, 3, 1, 2) for _ in range(2))
    else:
        a, b = pair((2, 3, rh, rw), rw)
    luma = R.LUMA_BT601 if form == "luma" else None
    got = measure(mctx, a, b, luma=luma, flags=S.METRIC_SSE)
    assert (got[..., 1] == rh * rw).all()
    check(got, reference(a, b, luma=luma, ssim=False), f"{rh} x {rw}, {form}, SSE only")


@pytest.mark.parametrize("rh,rw", [(1025, 3), (2052, 5)], ids=lambda v: str(v))
def test_finish_pass_over_more_than_256_sse_partials(mctx, rh, rw):
    lib = C.CDLL(str(S.tuning_library_path()))
    lim = (C.c_int * 4)()
    assert lib.srcnn_debug_metric_limits(lim) == 0
    assert -(-rh // lim[2]) in (257, 513), "one and two partials past the finish kernel's 256 threads"
    a, b = pair((2, 1, rh, rw), rh)
    check(measure(mctx, a, b, flags=S.METRIC_SSE), reference(a, b, ssim=False), f"{rh} x {rw}, SSE only")


@pytest.mark.parametrize("name", ["one-band-257-tiles", "17x16-tiles"])
def test_finish_pass_over_more_than_256_ssim_partials(mctx, name):
    T, B = tile()
    rh, rw = (13, 256 * T + 11) if name == "one-band-257-tiles" else (16 * B + 11, 15 * T + 11)
    n_bt, n_ct = -(-(rh - 10) // B), -(-(rw - 10) // T)
    assert (n_bt, n_ct) == ((1, 257) if name == "one-band-257-tiles" else (17, 16)) and n_bt * n_ct > 256
    a, b = pair((1, 1, rh, rw), rh + rw)
    got = measure(mctx, a, b, flags=S.METRIC_SSIM)
    assert got[0, 0, 3] == (rh - 10) * (rw - 10)
    check(got, reference(a, b, sse=False), f"{name} ({rh} x {rw}), SSIM only")


# ---- data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1.0, 255.0])
@pytest.mark.parametrize("data", ["noise", "smooth", "near-constant"])
def test_data_and_ranges(mctx, data, L):
    shape = (1, 1, 40, 70)
    if data == "noise":
        a, b = cuda(R.noise(shape, 1, L)), cuda(R.noise(shape, 2, L))
    elif data == "smooth":
        s = R.smooth(shape, 3, L)
        a, b = cuda(s), cuda(np.clip(s + 0.01 * L * np.random.default_rng(4).standard_normal(shape), 0, L).astype(np.float32))
    else:
        a, b = (cuda(x) for x in R.near_constant(shape, L))      # where a float32 E[x^2] - mu^2 cancels
    got = measure(mctx, a, b, border=2, L=L)
    check(got, reference(a, b, border=2, L=L), f"{data}, L = {L}")
    assert 0.0 < got[0, 0, 2] / got[0, 0, 3] < 1.0


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def test_padded_strides_and_pitches_one_element_off_the_base(mctx):
    n, c, h, w = 2, 3, 19, 26
    stride, ch_pitch, frame_pitch = w + 5, (w + 5) * h + 7, 3 * ((w + 5) * h + 7) + 11

    def padded(x):
        flat = torch.full((1 + n * frame_pitch,), 9.0, dtype=torch.float32, device="cuda")
        view = flat.as_strided((n, c, h, w), (frame_pitch, ch_pitch, stride, 1), 1)
        view.copy_(cuda(x))
        return view
    a, b = padded(R.noise((n, c, h, w), 5)), padded(R.smooth((n, c, h, w), 6))
    assert a.data_ptr() % 8 == 4 and not a.is_contiguous()
    check(measure(mctx, a, b, border=1), reference(a, b, border=1), "padded planes")


def test_hwc_uint8_against_channels_last_float16_of_the_same_picture(mctx):
    rng = np.random.default_rng(7)
    u8 = torch.from_numpy(rng.integers(0, 256, (2, 17, 31, 3), dtype=np.uint8)).cuda()
    a = u8.permute(0, 3, 1, 2)                                                    # N x H x W x 3 bytes, as decoded
    b = (a.float() / 255.0).to(torch.float16).contiguous(memory_format=torch.channels_last)
    got = measure(mctx, a, b)
    check(got, reference(a, b), "uint8 HWC against float16 channels_last")
    assert (got[..., 0] > 0).all() and (got[..., 2] / got[..., 3] > 0.999).all(), "only the float16 rounding lies between them"
    # the same bytes at scale 1 against themselves as float32: L = 255, and equal
    same = measure(mctx, a, a.float().contiguous(), L=255.0, in_scale=1.0)
    assert (same[..., 0] == 0).all() and np.array_equal(same[..., 2], same[..., 3])


def test_planar_bfloat16(mctx):
    a, b = pair((1, 3, 23, 15), 8)
    a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    check(measure(mctx, a, b, border=1), reference(a, b, border=1), "planar bfloat16")


def test_rgba_with_the_alpha_ignored(mctx):
    rng = np.random.default_rng(9)
    rgba_a = torch.from_numpy(rng.integers(0, 256, (14, 29, 4), dtype=np.uint8)).cuda()
    rgba_b = rgba_a.clone()
    rgba_b[..., :3] = torch.from_numpy(rng.integers(0, 256, (14, 29, 3), dtype=np.uint8)).cuda()
    a, b = rgba_a[..., :3].permute(2, 0, 1)[None], rgba_b[..., :3].permute(2, 0, 1)[None]
    got = measure(mctx, a, b)
    check(got, reference(a, b), "RGBA, three channels")
    rgba_b[..., 3] = 255 - rgba_b[..., 3]
    assert np.array_equal(measure(mctx, a, b).view(np.uint64), got.view(np.uint64)), "the alpha is never read"


@pytest.mark.parametrize("luma", [R.LUMA_BT601, (65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0, 16.0 / 255.0), (0.0, 1.0, 0.0, 0.0)])
def test_luma_mode_against_the_references_luma(mctx, luma):
    a, b = pair((2, 3, 21, 33), 10)
    b = b.contiguous(memory_format=torch.channels_last)
    got = measure(mctx, a, b, border=3, luma=luma)
    assert got.shape == (2, 1, 4)
    check(got, reference(a, b, border=3, luma=luma), f"luma {luma[:2]}")
    if luma == (0.0, 1.0, 0.0, 0.0):
        assert np.array_equal(got[:, 0].view(np.uint64), measure(mctx, a, b, border=3)[:, 1].view(np.uint64)), "the luma that is channel 1"


# ---- properties ------------------------------------------------------------------------------------------------------------
def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_identical_inputs_give_zero_and_exactly_one_per_window(mctx):
    T, B = tile()
    for shape, L, luma in (((2, 3, 30, T + 20), 1.0, None), ((1, 3, B + 15, 25), 255.0, R.LUMA_BT601), ((1, 1, 40, 70), 1.0, None)):
        x = cuda(R.near_constant(shape, L)[1]) if shape[1] == 1 else cuda(R.smooth(shape, 11, L))
        got = measure(mctx, x, x.clone(), border=2, luma=luma, L=L)
        assert (got[..., 0] == 0).all() and np.array_equal(got[..., 2], got[..., 3]) and (got[..., 3] > 0).all(), shape
        same_memory = measure(mctx, x, x, border=2, luma=luma, L=L)
        assert np.array_equal(u64(same_memory), u64(got))


def test_deterministic_batch_invariant_and_symmetric(mctx):
    T, B = tile()
    a, b = pair((3, 3, B + 14, T + 25), 12)
    got = measure(mctx, a, b, border=1)
    assert np.array_equal(u64(measure(mctx, a, b, border=1)), u64(got)), "the same call twice: the same 64-bit patterns"
    for f in range(3):
        one = measure(mctx, a[f:f + 1], b[f:f + 1], border=1)
        assert np.array_equal(u64(one[0]), u64(got[f])), f"frame {f} alone equals frame {f} of the batch"
    assert np.array_equal(u64(measure(mctx, b, a, border=1)), u64(got)), "a and b swapped"
    luma = measure(mctx, a, b, border=1, luma=R.LUMA_BT601)
    assert np.array_equal(u64(measure(mctx, b, a, border=1, luma=R.LUMA_BT601)), u64(luma))


def test_an_unselected_metric_is_zero_and_the_other_unchanged(mctx):
    a, b = pair((2, 3, 25, 31), 13)
    both = measure(mctx, a, b)
    sse, ssim = measure(mctx, a, b, flags=S.METRIC_SSE), measure(mctx, a, b, flags=S.METRIC_SSIM)
    assert (sse[..., 2:] == 0).all() and np.array_equal(u64(sse[..., :2]), u64(both[..., :2]))
    assert (ssim[..., :2] == 0).all() and np.array_equal(u64(ssim[..., 2:]), u64(both[..., 2:]))


def test_metric_psnr_from_the_sums(mctx):
    a, b = pair((1, 1, 20, 20), 14)
    got = measure(mctx, a, b, flags=S.METRIC_SSE)[0, 0]
    la, lb = loaded(a)[0, 0], loaded(b)[0, 0]
    assert S.metric_psnr(got[0], got[1], 1.0) == pytest.approx(10 * math.log10(1.0 / np.mean((la - lb) ** 2)), abs=1e-10)


# ---- the torch methods -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fast():
    m = compile_module(make_module(1, 1, "zeros", 3))      # a 1-channel module: the channel count comes from the tensors
    yield m
    m.close()


def torch_script(a, b, border, luma, L):
    """The usual script, in float64: conv2d with the same window on .double() tensors"""
    a, b = a.double(), b.double()
    if luma is not None:
        w = torch.tensor(luma, dtype=torch.float32, device=a.device).double()
        a, b = ((((w[0] * t[:, 0] + w[1] * t[:, 1]) + w[2] * t[:, 2]) + w[3]).unsqueeze(1) for t in (a, b))
    if border:
        a, b = a[..., border:-border, border:-border], b[..., border:-border, border:-border]
    n, c, h, w_ = a.shape
    g = torch.from_numpy(R.window()).to(a.device)
    win = torch.outer(g, g)[None, None].repeat(c, 1, 1, 1)
    blur = lambda t: F.conv2d(t, win, groups=c)
    ma, mb, eaa, ebb, eab = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    m = ((2 * ma * mb + c1) * (2 * (eab - ma * mb) + c2)) / ((ma * ma + mb * mb + c1) * ((eaa - ma * ma) + (ebb - mb * mb) + c2))
    mse = ((a - b) ** 2).mean(dim=(-2, -1))
    return 10 * torch.log10(L * L / mse), m.mean(dim=(-2, -1))


@pytest.mark.parametrize("side", [False, True], ids=["default-stream", "side-stream"])
def test_torch_methods_on_both_streams(fast, mctx, side):
    a, b = pair((2, 3, 27, 40), 15)
    b = b.to(torch.float16).contiguous(memory_format=torch.channels_last)
    want = measure(mctx, a, b, border=2, luma=R.LUMA_BT601)
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        m = fast.metrics(a, b, border=2, luma=R.LUMA_BT601)
        p = fast.psnr(a, b, border=2, luma=R.LUMA_BT601)
        s = fast.ssim(a, b, border=2, luma=R.LUMA_BT601)
        planes = fast.metrics(a, b, ssim=False)
    stream.synchronize()
    assert m.shape == (2, 1, 4) and m.dtype == torch.float64 and m.device == a.device and p.shape == s.shape == (2, 1)
    assert planes.shape == (2, 3, 4) and (planes[..., 2:] == 0).all()
    assert np.array_equal(u64(m.cpu().numpy()), u64(want)), "the torch method is the Context call"
    ps, ss = torch_script(a, b.float(), 2, R.LUMA_BT601, 1.0)
    assert torch.allclose(p, ps, rtol=0, atol=1e-9) and float((s - ss).abs().max()) <= R.SSIM_TOL
    assert torch.equal(s, m[..., 2] / m[..., 3])


def test_torch_psnr_is_inf_on_identical_inputs_and_uint8_reads_at_its_scale(fast):
    u8 = torch.from_numpy(np.random.default_rng(16).integers(0, 256, (1, 20, 24, 3), dtype=np.uint8)).cuda().permute(0, 3, 1, 2)
    assert torch.isinf(fast.psnr(u8, u8.clone())).all() and (fast.psnr(u8, u8.clone()) > 0).all()
    assert (fast.ssim(u8, u8.float() * (1.0 / 255.0)) == 1.0).all(), "a byte loads as x.float() * scale"
    noisy = (u8.float() + 2.0).clamp(0, 255)
    p255 = fast.psnr(u8, noisy, data_range=255.0, in_scale=1.0)
    ps, _ = torch_script(u8.float(), noisy, 0, None, 255.0)
    assert p255.shape == (1, 3) and torch.allclose(p255, ps, rtol=0, atol=1e-9)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_context_usable(mctx):
    lib, h = mctx._lib, mctx._h
    a, b = pair((1, 3, 16, 18), 17)
    one = a[:, :1].contiguous()
    ia, ib, i1 = describe_image(a, 3)[0], describe_image(b, 3)[0], describe_image(one, 1)[0]
    out = torch.full((12,), -7.25, dtype=torch.float64, device="cuda")
    good = measure(mctx, a, b)
    f4 = lambda *v: (C.c_float * 4)(*v)
    zero_step = S.Image(a.data_ptr(), S.ELEM_F32, 0, 18, 288, 0)
    bad_elem = S.Image(a.data_ptr(), 7, 1, 18, 288, 0)
    o = out.data_ptr()
    cases = {
        "descriptor a": (zero_step, ib, 18, 16, 3, 1, 0, None, 1.0, BOTH, o),
        "descriptor b": (ia, bad_elem, 18, 16, 3, 1, 0, None, 1.0, BOTH, o),
        "null descriptor": (None, ib, 18, 16, 3, 1, 0, None, 1.0, BOTH, o),
        "luma with one channel": (i1, i1, 18, 16, 1, 1, 0, f4(0.3, 0.6, 0.1, 0.0), 1.0, BOTH, o),
        "two channels": (ia, ib, 18, 16, 2, 1, 0, None, 1.0, BOTH, o),
        "non-finite luma": (ia, ib, 18, 16, 3, 1, 0, f4(0.3, math.nan, 0.1, 0.0), 1.0, BOTH, o),
        "infinite luma offset": (ia, ib, 18, 16, 3, 1, 0, f4(0.3, 0.6, 0.1, math.inf), 1.0, BOTH, o),
        "data_range 0": (ia, ib, 18, 16, 3, 1, 0, None, 0.0, BOTH, o),
        "data_range nan": (ia, ib, 18, 16, 3, 1, 0, None, math.nan, BOTH, o),
        "data_range inf": (ia, ib, 18, 16, 3, 1, 0, None, math.inf, BOTH, o),
        "negative border": (ia, ib, 18, 16, 3, 1, -1, None, 1.0, BOTH, o),
        "empty region": (ia, ib, 18, 16, 3, 1, 8, None, 1.0, S.METRIC_SSE, o),
        "region under 11 x 11": (ia, ib, 18, 16, 3, 1, 3, None, 1.0, BOTH, o),
        "flags 0": (ia, ib, 18, 16, 3, 1, 0, None, 1.0, 0, o),
        "unknown flag": (ia, ib, 18, 16, 3, 1, 0, None, 1.0, 4 | S.METRIC_SSE, o),
        "null output": (ia, ib, 18, 16, 3, 1, 0, None, 1.0, BOTH, None),
        "no frames": (ia, ib, 18, 16, 3, 0, 0, None, 1.0, BOTH, o),
    }
    for name, (xa, xb, *rest) in cases.items():
        pa = C.byref(xa.c()) if xa is not None else None
        rc = lib.srcnn_metrics_image_dev(h, pa, C.byref(xb.c()), *rest)
        assert rc == S.ERR_INVALID, name
        assert b"metrics_image_dev" in lib.srcnn_last_error(h), name
        mctx.synchronize()
        assert (out == -7.25).all(), f"{name}: a refused call launches nothing"
        assert np.array_equal(u64(measure(mctx, a, b)), u64(good)), f"{name}: the context is usable afterwards"
    # the squared error of the 2 x 4 region that is too small for a window is a good call
    check(measure(mctx, a, b, border=6, flags=S.METRIC_SSE), reference(a, b, border=6, ssim=False), "border 6, SSE only")
