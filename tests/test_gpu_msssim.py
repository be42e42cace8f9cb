"""MS-SSIM on the GPU (srcnn_msssim_image_dev, CompiledModule.msssim_sums / msssim) against the numpy float64 statement of
tests/msssim_reference.py.  All planes are small.

Tolerance: per scale, |cs_sum / n_win - reference| and |ssim_sum / n_win - reference| <= SSIM_TOL = 1e-9, the project's figure
for this window arithmetic (tests/metrics_reference.py): each factor of a window carries a few dozen roundings of 2^-53 on
quantities <= 2 L^2 against C1 = 1e-4 L^2.  The pyramid adds three float64 additions and an exact scaling per pixel and scale,
which the statement performs in the same order, so the scales >= 1 start from the same bits as the statement's."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.torch_api import compile_module, describe_image
import metrics_reference as R
import msssim_reference as M
from test_gpu_resize_f32 import make_module

pytestmark = pytest.mark.gpu

GUARD = 4          # doubles either side of d_out


@functools.lru_cache(maxsize=None)
def tile():
    """(T, B0, B1): window columns of one workgroup of the window kernel and its window rows at scale 0 and at the scales >= 1,
    from the tuning library's hook"""
    lib = C.CDLL(str(S.tuning_library_path()))
    out = (C.c_int * 5)()
    assert lib.srcnn_debug_msssim_limits(out) == 0
    return out[0], out[1], out[2]


@pytest.fixture(scope="module")
def mctx():
    ctx = S.Context(0)          # no model: the metric needs none
    yield ctx
    ctx.close()


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def loaded(t, in_scale=None):
    """What the library loads from a tensor (N, C, H, W), as float64 numpy"""
    if t.dtype == torch.uint8:
        return R.load(t.cpu().numpy(), in_scale)
    return t.float().cpu().numpy().astype(np.float64)      # float16 and bfloat16 widen exactly


def measure(ctx, a, b, border=0, luma=None, L=1.0, n_scales=5, in_scale=None):
    """srcnn_msssim_image_dev on two CUDA tensors (N, C, H, W) as they lie -> (N, P, S, 3) float64 numpy; the output sits
    between guards, which must come back untouched"""
    n, c, h, w = a.shape
    ia, ib = describe_image(a, c, in_scale)[0], describe_image(b, c, in_scale)[0]
    per_frame = 1 if luma is not None else c
    out = torch.full((n * per_frame * n_scales * 3 + 2 * GUARD,), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.msssim_image_dev(ia, ib, w, h, c, n, border, luma, L, n_scales, out.data_ptr() + 8 * GUARD)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == -7.25).all() and (got[-GUARD:] == -7.25).all(), "d_out is written inside its bounds only"
    return got[GUARD:-GUARD].reshape(n, per_frame, n_scales, 3)


def reference(a, b, border=0, luma=None, L=1.0, n_scales=5, in_scale=None):
    la, lb = loaded(a, in_scale), loaded(b, in_scale)
    return np.stack([M.msssim_sums(la[f], lb[f], border=border, luma=luma, data_range=L, n_scales=n_scales) for f in range(la.shape[0])])


def check(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got[..., 2], ref[..., 2]), "n_win"
    cs_err = float(np.abs(got[..., 0] / got[..., 2] - ref[..., 0] / ref[..., 2]).max())
    ssim_err = float(np.abs(got[..., 1] / got[..., 2] - ref[..., 1] / ref[..., 2]).max())
    print(f"{what}: |mean cs - reference| {cs_err:.3g}, |mean SSIM - reference| {ssim_err:.3g} over {got.shape[-2]} scales")
    assert cs_err <= R.SSIM_TOL and ssim_err <= R.SSIM_TOL
    return max(cs_err, ssim_err)


def pair(shape, seed, L=1.0):
    return cuda(R.noise(shape, seed, L)), cuda(R.smooth(shape, seed + 1, L))


def noisy_pair(shape, seed, L=1.0, sigma=0.05):
    a = R.smooth(shape, seed, L)
    b = np.clip(a + sigma * L * np.random.default_rng(seed + 100).standard_normal(shape), 0.0, L).astype(np.float32)
    return cuda(a), cuda(b)


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [0, 3])
@pytest.mark.parametrize("rh,rw", [(161, 161), (163, 171), (161, 230), (176, 192)], ids=lambda v: str(v))
def test_five_scales(mctx, rh, rw, border):
    """161 x 161: one window at the top scale; 163 x 171: odd at several levels (163 -> 82 -> 41 -> 21 -> 11, 171 -> 86 -> 43 -> 22
    -> 11); 161 x 230: several column tiles at scale 0; 176 x 192: even throughout.  The picture grows by twice the border."""
    a, b = pair((1, 1, rh + 2 * border, rw + 2 * border), rh + rw)
    got = measure(mctx, a, b, border=border)
    assert got[0, 0, :, 2].tolist() == [float((-(-rh // 2 ** s) - 10) * (-(-rw // 2 ** s) - 10)) for s in range(5)]
    if (rh, rw) == (161, 161):
        assert got[0, 0, :, 2].tolist() == [22801, 5041, 961, 121, 1]
    check(got, reference(a, b, border=border), f"{rh} x {rw}, border {border}")


def level1_case(name, odd):
    """(h', w') whose LEVEL-1 plane has the named count of window columns or rows; `odd`: the level-0 size is odd"""
    T, _, B = tile()
    kind, expr = name.split("=")
    n = eval(expr, {"T": T, "B": B}) + 10                  # the level-1 side
    side = 2 * n - (1 if odd else 0)                       # ceil(side / 2) == n
    return (25 if odd else 26, side) if kind == "cols" else (side, 45 if odd else 46)


LEVEL1 = ["cols=T-1", "cols=T", "cols=T+1", "cols=2*T+1", "rows=B-1", "rows=B", "rows=B+1"]


@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
@pytest.mark.parametrize("name", LEVEL1)
def test_two_scales_on_the_level_1_tile_bounds(mctx, name, odd):
    rh, rw = level1_case(name, odd)
    a, b = pair((1, 1, rh, rw), rh + rw)
    got = measure(mctx, a, b, n_scales=2)
    h1, w1 = -(-rh // 2), -(-rw // 2)
    assert got[0, 0, 1, 2] == (h1 - 10) * (w1 - 10) and (rh % 2 == 1) == odd and (rw % 2 == 1) == odd
    check(got, reference(a, b, n_scales=2), f"{name}, {'odd' if odd else 'even'} ({rh} x {rw}; level 1 {h1} x {w1})")


@pytest.mark.parametrize("name", ["cols=T-1", "cols=T", "cols=T+1", "rows=B-1", "rows=B", "rows=B+1", "rows=2*B+1"])
def test_one_scale_on_the_scale_0_tile_bounds(mctx, name):
    T, B, _ = tile()
    kind, expr = name.split("=")
    n = eval(expr, {"T": T, "B": B}) + 10
    rh, rw = (13, n) if kind == "cols" else (n, 23)
    a, b = pair((1, 1, rh + 2, rw + 2), rh + rw)
    got = measure(mctx, a, b, border=1, n_scales=1)
    assert got[0, 0, 0, 2] == (rh - 10) * (rw - 10)
    check(got, reference(a, b, border=1, n_scales=1), f"{name} at scale 0 ({rh} x {rw})")


def test_the_hook_reports_a_tile_the_shapes_cross():
    T, B0, B = tile()
    assert 1 < T <= 64 and B > 1 and B0 > 1
    assert level1_case("cols=T+1", False) == (26, 2 * (T + 11)) and level1_case("rows=B-1", True) == (2 * (B + 9) - 1, 45)


def test_one_scale_is_the_existing_ssim(mctx):
    a, b = pair((2, 3, 40, 75), 3)
    got = measure(mctx, a, b, border=1, n_scales=1)
    la, lb = loaded(a), loaded(b)
    ref = np.stack([R.metrics(la[f], lb[f], border=1, sse=False) for f in range(2)])      # (N, P, 4)
    assert got.shape == (2, 3, 1, 3) and np.array_equal(got[..., 0, 2], ref[..., 3])
    err = float(np.abs(got[..., 0, 1] / got[..., 0, 2] - ref[..., 2] / ref[..., 3]).max())
    print(f"S = 1: |mean SSIM - metrics_reference| {err:.3g}")
    assert err <= R.SSIM_TOL


# ---- data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1.0, 255.0])
@pytest.mark.parametrize("data", ["noise", "smooth", "near-constant"])
def test_data_and_ranges(mctx, data, L):
    shape = (1, 1, 165, 170)
    if data == "noise":
        a, b = cuda(R.noise(shape, 1, L)), cuda(R.noise(shape, 2, L))
    elif data == "smooth":
        a, b = noisy_pair(shape, 3, L)
    else:
        a, b = (cuda(x) for x in R.near_constant(shape, L))      # where a float32 E[x^2] - mu^2 cancels
    got = measure(mctx, a, b, border=2, L=L)
    check(got, reference(a, b, border=2, L=L), f"{data}, L = {L}")
    if data == "smooth":
        assert ((got[0, 0, :, 0] / got[0, 0, :, 2]) > 0.5).all()


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def test_padded_strides_and_pitches_one_element_off_the_base(mctx):
    n, c, h, w = 2, 3, 163, 166
    stride, ch_pitch, frame_pitch = w + 5, (w + 5) * h + 7, 3 * ((w + 5) * h + 7) + 11

    def padded(x):
        flat = torch.full((1 + n * frame_pitch,), 9.0, dtype=torch.float32, device="cuda")
        view = flat.as_strided((n, c, h, w), (frame_pitch, ch_pitch, stride, 1), 1)
        view.copy_(cuda(x))
        return view
    a, b = padded(R.noise((n, c, h, w), 5)), padded(R.smooth((n, c, h, w), 6))
    assert a.data_ptr() % 8 == 4 and not a.is_contiguous()
    check(measure(mctx, a, b, border=1), reference(a, b, border=1), "padded planes")


def test_hwc_uint8_with_a_luma_against_channels_last_float16_of_the_same_picture(mctx):
    rng = np.random.default_rng(7)
    u8 = torch.from_numpy(rng.integers(0, 256, (2, 162, 165, 3), dtype=np.uint8)).cuda()
    a = u8.permute(0, 3, 1, 2)                                                    # N x H x W x 3 bytes, as decoded
    b = (a.float() / 255.0).to(torch.float16).contiguous(memory_format=torch.channels_last)
    got = measure(mctx, a, b, luma=R.LUMA_BT601)
    assert got.shape == (2, 1, 5, 3)
    check(got, reference(a, b, luma=R.LUMA_BT601), "uint8 HWC against float16 channels_last, BT.601 luma")
    assert (got[..., 0] / got[..., 2] > 0.99).all(), "only the float16 rounding lies between them"
    # the same bytes at scale 1 against themselves as float32: L = 255, and equal
    same = measure(mctx, a, a.float().contiguous(), L=255.0, in_scale=1.0, luma=R.LUMA_BT601)
    assert np.array_equal(same[..., 0], same[..., 2]) and np.array_equal(same[..., 1], same[..., 2])


def test_planar_bfloat16(mctx):
    a, b = pair((1, 3, 163, 161), 8)
    a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    check(measure(mctx, a, b, border=1, n_scales=4), reference(a, b, border=1, n_scales=4), "planar bfloat16")


# ---- properties ------------------------------------------------------------------------------------------------------------
def test_frames_and_channels_against_separate_calls_bit_for_bit(mctx):
    a, b = pair((2, 3, 165, 172), 12)
    got = measure(mctx, a, b, border=1)
    assert got.shape == (2, 3, 5, 3)
    for f in range(2):
        one = measure(mctx, a[f:f + 1], b[f:f + 1], border=1)
        assert np.array_equal(u64(one[0]), u64(got[f])), f"frame {f} alone equals frame {f} of the batch"
        for ch in range(3):
            plane = measure(mctx, a[f:f + 1, ch:ch + 1], b[f:f + 1, ch:ch + 1], border=1)
            assert np.array_equal(u64(plane[0, 0]), u64(got[f, ch])), f"plane {ch} of frame {f} alone"
    check(got, reference(a, b, border=1), "2 frames x 3 channels")


def test_deterministic_and_symmetric(mctx):
    a, b = pair((2, 3, 163, 171), 13)
    for luma in (None, R.LUMA_BT601):
        got = measure(mctx, a, b, border=1, luma=luma)
        assert np.array_equal(u64(measure(mctx, a, b, border=1, luma=luma)), u64(got)), "the same call twice: the same 64-bit patterns"
        assert np.array_equal(u64(measure(mctx, b, a, border=1, luma=luma)), u64(got)), "a and b swapped"


def test_identical_pictures_give_exactly_n_win(mctx):
    for shape, L, luma in (((2, 3, 163, 171), 1.0, None), ((1, 3, 161, 180), 255.0, R.LUMA_BT601), ((1, 1, 170, 161), 1.0, None)):
        x = cuda(R.near_constant(shape, L)[1]) if shape[1] == 1 else cuda(R.smooth(shape, 11, L))
        got = measure(mctx, x, x.clone(), luma=luma, L=L)
        assert np.array_equal(got[..., 0], got[..., 2]) and np.array_equal(got[..., 1], got[..., 2]) and (got[..., 2] > 0).all(), shape
        assert np.array_equal(u64(measure(mctx, x, x, luma=luma, L=L)), u64(got)), "the same memory twice"


# ---- the torch methods -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fast():
    m = compile_module(make_module(1, 1, "zeros", 3))      # a 1-channel module: the channel count comes from the tensors
    yield m
    m.close()


@pytest.mark.parametrize("side", [False, True], ids=["default-stream", "side-stream"])
def test_torch_methods_on_both_streams(fast, mctx, side):
    a, b = noisy_pair((2, 3, 166, 170), 15)
    b = b.to(torch.float16).contiguous(memory_format=torch.channels_last)
    want = measure(mctx, a, b, border=2, luma=R.LUMA_BT601)
    want3 = measure(mctx, a, b, n_scales=3)
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        sums = fast.msssim_sums(a, b, border=2, luma=R.LUMA_BT601)
        value = fast.msssim(a, b, border=2, luma=R.LUMA_BT601)
        sums3 = fast.msssim_sums(a, b, n_scales=3)
        value3 = fast.msssim(a, b, n_scales=3, weights=(0.2, 0.3, 0.5))
    stream.synchronize()
    assert sums.shape == (2, 1, 5, 3) and sums.dtype == torch.float64 and sums.device == a.device and value.shape == (2, 1)
    assert sums3.shape == (2, 3, 3, 3) and value3.shape == (2, 3) and value3.dtype == torch.float64
    assert np.array_equal(u64(sums.cpu().numpy()), u64(want)), "the torch method is the Context call"
    assert np.array_equal(u64(sums3.cpu().numpy()), u64(want3))
    for f in range(2):
        host = S.metric_msssim(want[f, 0])
        assert 0.5 < host < 1.0 and abs(float(value[f, 0]) - host) <= 1e-14 * host
        for p in range(3):
            host3 = S.metric_msssim(want3[f, p], (0.2, 0.3, 0.5))
            assert abs(float(value3[f, p]) - host3) <= 1e-14 * host3
    assert abs(S.metric_msssim(want[0, 0]) - M.msssim_value(reference(a, b, border=2, luma=R.LUMA_BT601)[0, 0])) <= 1e-8


def test_torch_msssim_clamps_at_zero_and_reads_uint8_at_its_scale(fast):
    u8 = torch.from_numpy(np.random.default_rng(16).integers(0, 256, (1, 161, 164, 3), dtype=np.uint8)).cuda().permute(0, 3, 1, 2)
    assert (fast.msssim(u8, u8.float() * (1.0 / 255.0)) == 1.0).all(), "a byte loads as x.float() * scale"
    inverted = 255 - u8                    # negative covariance at every scale: a mean cs below 0, a product of exactly 0
    sums = fast.msssim_sums(u8, inverted).cpu().numpy()
    assert (sums[..., 0] < 0).any()
    value = fast.msssim(u8, inverted).cpu().numpy()
    for p in range(3):
        assert value[0, p] == 0.0 and S.metric_msssim(sums[0, p]) == 0.0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_context_usable(mctx):
    lib, h = mctx._lib, mctx._h
    a, b = pair((1, 3, 166, 168), 17)
    one = a[:, :1].contiguous()
    ia, ib, i1 = describe_image(a, 3)[0], describe_image(b, 3)[0], describe_image(one, 1)[0]
    out = torch.full((3 * 5 * 3,), -7.25, dtype=torch.float64, device="cuda")
    good = measure(mctx, a, b)
    f4 = lambda *v: (C.c_float * 4)(*v)
    zero_step = S.Image(a.data_ptr(), S.ELEM_F32, 0, 168, 166 * 168, 0)
    bad_elem = S.Image(a.data_ptr(), 7, 1, 168, 166 * 168, 0)
    o = out.data_ptr()
    cases = {
        "descriptor a": (zero_step, ib, 168, 166, 3, 1, 0, None, 1.0, 5, o),
        "descriptor b": (ia, bad_elem, 168, 166, 3, 1, 0, None, 1.0, 5, o),
        "null descriptor": (None, ib, 168, 166, 3, 1, 0, None, 1.0, 5, o),
        "luma with one channel": (i1, i1, 168, 166, 1, 1, 0, f4(0.3, 0.6, 0.1, 0.0), 1.0, 5, o),
        "two channels": (ia, ib, 168, 166, 2, 1, 0, None, 1.0, 5, o),
        "non-finite luma": (ia, ib, 168, 166, 3, 1, 0, f4(0.3, math.nan, 0.1, 0.0), 1.0, 5, o),
        "data_range 0": (ia, ib, 168, 166, 3, 1, 0, None, 0.0, 5, o),
        "data_range nan": (ia, ib, 168, 166, 3, 1, 0, None, math.nan, 5, o),
        "negative border": (ia, ib, 168, 166, 3, 1, -1, None, 1.0, 5, o),
        "empty region": (ia, ib, 168, 166, 3, 1, 83, None, 1.0, 1, o),
        "n_scales 0": (ia, ib, 168, 166, 3, 1, 0, None, 1.0, 0, o),
        "n_scales 6": (ia, ib, 168, 166, 3, 1, 0, None, 1.0, 6, o),
        "n_scales -1": (ia, ib, 168, 166, 3, 1, 0, None, 1.0, -1, o),
        "null output": (ia, ib, 168, 166, 3, 1, 0, None, 1.0, 5, None),
        "no frames": (ia, ib, 168, 166, 3, 0, 0, None, 1.0, 5, o),
    }
    # each minimum size: a region one short of 10 * 2^(S - 1) + 1 in its height (166 rows) and, with narrower pictures, its width
    for s in range(1, 6):
        border = (166 - (M.min_side(s) - 1)) // 2
        assert 166 - 2 * border == M.min_side(s) - 1 and 168 - 2 * border >= M.min_side(s)
        cases[f"S = {s}: region one row short"] = (ia, ib, 168, 166, 3, 1, border, None, 1.0, s, o)
        width = M.min_side(s) - 1 + 2 * 2
        cases[f"S = {s}: region one column short"] = (ia, ib, width, 166, 3, 1, 2, None, 1.0, s, o)
    for name, (xa, xb, *rest) in cases.items():
        pa = C.byref(xa.c()) if xa is not None else None
        rc = lib.srcnn_msssim_image_dev(h, pa, C.byref(xb.c()), *rest)
        assert rc == S.ERR_INVALID, name
        message = lib.srcnn_last_error(h)
        assert b"msssim_image_dev" in message, name
        if name.startswith("S = "):
            s = rest[-2]
            assert f"{s} scales need a region of at least {M.min_side(s)} x {M.min_side(s)}".encode() in message, message
        mctx.synchronize()
        assert (out == -7.25).all(), f"{name}: a refused call launches nothing"
        assert np.array_equal(u64(measure(mctx, a, b)), u64(good)), f"{name}: the context is usable afterwards"
    # the smallest regions themselves are good calls
    for s in (1, 2):
        side = M.min_side(s)
        x, y = pair((1, 1, side, side), 18 + s)
        got = measure(mctx, x, y, n_scales=s)
        assert got[0, 0, s - 1, 2] == 1
        check(got, reference(x, y, n_scales=s), f"the smallest region of {s} scales")
