"""The float32 cubic resize on the GPU (srcnn_resize_cubic_f32(_dev), srcnn_process_f32(_dev), CompiledModule.resize / upscale):
both kernel forms against the float64 restatement and against torch's CPU result, exactness, layouts, resize + model against
the two calls made separately, the torch front end on both kinds of stream, refusals.  All planes are small."""
import ctypes as C

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.torch_api import compile_module
from color_reference import random_color_model
from resize_f32_reference import CASES, TOL, WIDTH_CASES, case, ref64, uniform
from spatial_reference import random_model

pytestmark = pytest.mark.gpu

MODES = [S.MODE_MFMA, S.MODE_BANDED16]
GUARD = float("nan")

_tuning = None


def hooks():
    """The tuning build's host-only hooks: which form a geometry reaches, and the tile sizes the kernel was compiled with."""
    global _tuning
    if _tuning is None:
        _tuning = C.CDLL(str(S.tuning_library_path()))
        _tuning.srcnn_debug_resize_f32_variant.argtypes = [C.c_int] * 4
        _tuning.srcnn_debug_resize_f32_limits.argtypes = [C.POINTER(C.c_int)]
    return _tuning


def tiled(sh, sw, dh, dw):
    return hooks().srcnn_debug_resize_f32_variant(sw, sh, dw, dh) == 1


def tile_rows():
    out = (C.c_int * 4)()
    assert hooks().srcnn_debug_resize_f32_limits(out) == 0
    return out[0]


RT = 16      # asserted against the hook in test_height_cases_sit_on_the_tile_bounds
HEIGHT_CASES = [(9, 21, dh, 40) for dh in (RT - 1, RT, RT + 1, 2 * RT - 1, 2 * RT, 2 * RT + 1)]


@pytest.fixture(scope="module")
def rctx():
    ctx = S.Context(0)          # no model: the resize needs none
    yield ctx
    ctx.close()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def resize_dev(ctx, x, dh, dw):
    """srcnn_resize_cubic_f32_dev on a contiguous CUDA tensor (N, C, H, W), on the context's own stream."""
    n, c, h, w = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32
    out = torch.full((n, c, dh, dw), GUARD, dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()
    ctx.resize_cubic_f32_dev(x.data_ptr(), w, h * w, c * h * w, w, h, out.data_ptr(), dw, dh * dw, c * dh * dw, dw, dh, c, n)
    ctx.synchronize()
    return out


def resize_plane(ctx, x, dh, dw):
    """One float32 numpy plane through the device form -> numpy."""
    return resize_dev(ctx, torch.from_numpy(np.array(x, dtype=np.float32))[None, None].cuda(), dh, dw)[0, 0].cpu().numpy()


# ---- accuracy: both forms against ref64 and against torch ------------------------------------------------------------------
def test_height_cases_sit_on_the_tile_bounds():
    assert tile_rows() == RT
    assert all(tiled(*c) for c in HEIGHT_CASES + WIDTH_CASES)


def test_the_selection_function_sends_the_cases_to_both_forms():
    assert not tiled(200, 300, 9, 7), "200x300 -> 9x7 is far outside a tile's span: the direct form"
    assert not tiled(23, 29, 11, 13)
    assert tiled(5, 4, 10, 8) and tiled(31, 67, 62, 134) and tiled(64, 250, 97, 511) and tiled(40, 300, 120, 900)


@pytest.mark.parametrize("sh,sw,dh,dw", CASES + WIDTH_CASES + HEIGHT_CASES, ids=lambda v: str(v))
def test_against_the_restatement_and_against_torch(rctx, sh, sw, dh, dw):
    x, ref, tor = case(sh, sw, dh, dw)
    got = resize_plane(rctx, x, dh, dw)
    assert got.dtype == np.float32 and got.shape == (dh, dw)
    tol = TOL * float(np.abs(x).max())
    err = np.abs(got.astype(np.float64) - ref).max()
    drift = np.abs(tor.astype(np.float64) - ref).max()          # torch's own float32 coordinate error, from the references alone
    err_t = np.abs(got.astype(np.float64) - tor.astype(np.float64)).max()
    print(f"{sh}x{sw} -> {dh}x{dw} ({'tiled' if tiled(sh, sw, dh, dw) else 'direct'}): |got - ref64| = {err:.3g} (tol {tol:.3g}), "
          f"|got - torch| = {err_t:.3g} (tol + {drift:.3g})")
    assert err <= tol
    assert err_t <= tol + drift


# ---- exactness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (33, 300)])
def test_same_size_is_an_exact_copy(rctx, h, w):
    x = uniform((h, w), 11) * np.float32(3.0) - np.float32(1.0)
    assert tiled(h, w, h, w)
    assert same_bits(resize_plane(rctx, x, h, w), x)


@pytest.mark.parametrize("sh,sw,dh,dw", [(5, 4, 10, 8), (17, 33, 25, 49), (200, 300, 9, 7)])
def test_constant_plane_stays_constant(rctx, sh, sw, dh, dw):
    v = np.float32(0.7314)
    got = resize_plane(rctx, np.full((sh, sw), v, np.float32), dh, dw)
    assert np.abs(got.astype(np.float64) - np.float64(v)).max() <= TOL * float(v)


# ---- layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,sw,dh,dw", [(17, 33, 25, 49), (40, 150, 33, 300), (60, 90, 9, 7)])
def test_channels_and_frames_equal_single_planes(rctx, sh, sw, dh, dw):
    x = torch.from_numpy(uniform((3, 3, sh, sw), 21)).cuda()
    got = resize_dev(rctx, x, dh, dw)
    assert not torch.isnan(got).any()
    for f in range(3):
        for c in range(3):
            one = resize_dev(rctx, x[f, c][None, None].contiguous(), dh, dw)
            assert same_bits(got[f, c], one[0, 0]), (f, c)


@pytest.mark.parametrize("dst_off,dst_pad", [(1, 9), (3, 8), (4, 12), (2, 11)])
@pytest.mark.parametrize("sh,sw,dh,dw", [(17, 33, 25, 49), (20, 130, 40, 260), (60, 90, 9, 7)])
def test_strided_views_in_guarded_tensors(rctx, sh, sw, dh, dw, dst_off, dst_pad):
    """Source and destination as windows of larger NaN-filled tensors at odd element offsets.  A destination row starts at
    float (1 + y) * (dw + dst_pad) + dst_off of its plane: with (4, 12) on 260 columns every row is 16-byte aligned (the vector
    stores), with the odd pitches the alignment changes from row to row (both store paths in one launch), with (3, 8) on 260
    columns no row is aligned (scalar stores only).  Same bits as contiguous tensors, guards untouched."""
    n, c = 2, 2
    x = torch.from_numpy(uniform((n, c, sh, sw), 31))
    want = resize_dev(rctx, x.cuda(), dh, dw)
    src_parent = torch.full((n, c, sh + 5, sw + 7), GUARD)
    src_parent[:, :, 2:2 + sh, 3:3 + sw] = x
    src_parent = src_parent.cuda()
    src = src_parent[:, :, 2:2 + sh, 3:3 + sw]
    dst_parent = torch.full((n, c, dh + 3, dw + dst_pad), GUARD, device="cuda")
    dst = dst_parent[:, :, 1:1 + dh, dst_off:dst_off + dw]
    assert dst_off + dw <= dw + dst_pad
    torch.cuda.synchronize()
    rctx.resize_cubic_f32_dev(src.data_ptr(), src.stride(2), src.stride(1), src.stride(0), sw, sh,
                              dst.data_ptr(), dst.stride(2), dst.stride(1), dst.stride(0), dw, dh, c, n)
    rctx.synchronize()
    assert same_bits(dst.contiguous(), want)
    outside = torch.ones_like(dst_parent, dtype=torch.bool)
    outside[:, :, 1:1 + dh, dst_off:dst_off + dw] = False
    assert torch.isnan(dst_parent[outside]).all(), "the floats around the destination window stay untouched"


@pytest.mark.parametrize("sh,sw,dh,dw", [(17, 33, 25, 49), (31, 67, 62, 134), (60, 90, 9, 7)])
def test_host_form_equals_device_form(rctx, sh, sw, dh, dw):
    x = uniform((3, sh, sw), 41)
    want = resize_dev(rctx, torch.from_numpy(x)[None].cuda(), dh, dw)[0].cpu().numpy()
    assert same_bits(rctx.resize_cubic_f32(x, dw, dh), want)
    assert same_bits(rctx.resize_cubic_f32(x[1], dw, dh), want[1])                       # (H, W) in, (H, W) out
    wide = np.full((3, sh + 2, sw + 5), np.float32(GUARD))
    wide[:, 1:1 + sh, 2:2 + sw] = x
    assert same_bits(rctx.resize_cubic_f32(wide[:, 1:1 + sh, 2:2 + sw], dw, dh), want)   # a strided host view, read in place


# ---- resize + model --------------------------------------------------------------------------------------------------------
PROCESS_SHAPES = [(17, 33, 25, 49), (20, 24, 40, 48)]        # the second needs more workspace than the first


def load(ctx, channels, padding, f2, mode):
    ctx.set_model(*(random_color_model(f2, 3) if channels == 3 else random_model(f2, 3)))
    ctx.set_padding(padding)
    ctx.set_mode(mode)
    ctx.set_input_range(2.0)          # [0, 1] data, and the overshoot of the resize


def process_dev(ctx, x, dh, dw):
    n, c, h, w = x.shape
    out = torch.full((n, c, dh, dw), GUARD, dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()
    ctx.process_f32_dev(x.data_ptr(), w, h * w, c * h * w, w, h, out.data_ptr(), dw, dh * dw, c * dh * dw, dw, dh, n)
    ctx.synchronize()
    return out


def forward_dev(ctx, x):
    n, c, h, w = x.shape
    out = torch.full_like(x, GUARD)
    torch.cuda.synchronize()
    ctx.forward_f32_dev(x.data_ptr(), w, h * w, c * h * w, out.data_ptr(), w, h * w, c * h * w, w, h, n)
    ctx.synchronize()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f2", [1, 5])
@pytest.mark.parametrize("padding", ["replicate", "zero"])
@pytest.mark.parametrize("channels", [1, 3])
def test_process_equals_resize_then_forward(channels, padding, f2, mode):
    """srcnn_process_f32_dev against the two calls made separately, bit for bit, on two frames; and one context running both
    shapes one after the other -- the second grows the workspace -- against a fresh context per shape."""
    xs = [torch.from_numpy(uniform((2, channels, sh, sw), 50 + sh)).cuda() for sh, sw, _, _ in PROCESS_SHAPES]
    with S.Context(0) as ctx:
        load(ctx, channels, padding, f2, mode)
        seq = [process_dev(ctx, x, dh, dw) for x, (_, _, dh, dw) in zip(xs, PROCESS_SHAPES)]
        for x, got, (_, _, dh, dw) in zip(xs, seq, PROCESS_SHAPES):
            assert got.shape == (2, channels, dh, dw) and torch.isfinite(got).all()
            assert same_bits(got, forward_dev(ctx, resize_dev(ctx, x, dh, dw)))
        # the host-memory form: one image, the same bits
        host = ctx.process_f32(xs[0][1].cpu().numpy(), PROCESS_SHAPES[0][3], PROCESS_SHAPES[0][2])
        assert same_bits(host, seq[0][1])
        if channels == 1:
            assert same_bits(ctx.process_f32(xs[0][1, 0].cpu().numpy(), PROCESS_SHAPES[0][3], PROCESS_SHAPES[0][2]), seq[0][1, 0])
    for x, got, (_, _, dh, dw) in zip(xs, seq, PROCESS_SHAPES):
        with S.Context(0) as fresh:
            load(fresh, channels, padding, f2, mode)
            assert same_bits(process_dev(fresh, x, dh, dw), got)


# ---- the torch front end ---------------------------------------------------------------------------------------------------
class SRCNN(torch.nn.Module):
    def __init__(self, channels, f2, padding_mode):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(channels, 64, 9, padding=4, padding_mode=padding_mode)
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=f2 // 2, padding_mode=padding_mode)
        self.conv3 = torch.nn.Conv2d(32, channels, 5, padding=2, padding_mode=padding_mode)

    def forward(self, x):
        return self.conv3(torch.relu(self.conv2(torch.relu(self.conv1(x)))))


def make_module(channels, f2, padding_mode, seed):
    torch.manual_seed(seed)
    return SRCNN(channels, f2, padding_mode).eval()


@pytest.mark.parametrize("channels,padding_mode,mode", [(1, "zeros", S.MODE_MFMA), (3, "replicate", S.MODE_MFMA),
                                                        (3, "zeros", S.MODE_BANDED16)])
def test_upscale_equals_resize_then_call(channels, padding_mode, mode):
    net = make_module(channels, 3, padding_mode, 5)
    fast = compile_module(net, mode=mode, input_range=2.0)
    try:
        x = torch.from_numpy(uniform((2, channels, 21, 30), 61)).cuda()
        by_scale = fast.upscale(x, scale=2)
        assert by_scale.shape == (2, channels, 42, 60) and by_scale.dtype == torch.float32 and by_scale.device == x.device
        two_steps = fast(fast.resize(x, (42, 60)))
        assert same_bits(by_scale, two_steps)
        by_size = fast.upscale(x, size=(31, 47))
        assert by_size.shape == (2, channels, 31, 47)
        assert same_bits(by_size, fast(fast.resize(x, (31, 47))))
        assert fast.upscale(x, scale=1.5).shape == (2, channels, 31, 45)          # (int)(21 * 1.5), (int)(30 * 1.5)
        one = fast.upscale(x[1], scale=2)                                          # (C, H, W) in, (C, H', W') out
        assert one.shape == (channels, 42, 60) and same_bits(one, by_scale[1])
        # the resize alone against the restatement (the model on float planes has its own tests: tests/test_gpu_f32.py)
        xn = x.cpu().numpy()
        r = fast.resize(x, (31, 47)).cpu().numpy()
        assert np.abs(r - ref64(xn, 31, 47)).max() <= TOL * float(np.abs(xn).max())
    finally:
        fast.close()


def test_upscale_on_a_non_default_stream_and_on_the_default_stream():
    net = make_module(1, 1, "zeros", 6)
    fast = compile_module(net, input_range=2.0)
    try:
        x = torch.from_numpy(uniform((2, 1, 40, 52), 71)).cuda()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            y = fast.upscale(x, scale=2)
            z = y * 2.0 + 1.0                         # the next torch op on that stream consumes the result unsynchronised
            r = fast.resize(x, (80, 104))
        stream.synchronize()
        assert same_bits(z, y * 2.0 + 1.0), "the op queued behind the call saw the finished result"
        # the default stream, interleaved with torch's own work on it
        yd = fast.upscale(x * 1.0, scale=2)
        zd = yd * 2.0 + 1.0
        rd = fast.resize(x * 1.0, (80, 104))
        torch.cuda.synchronize()
        assert same_bits(yd, y) and same_bits(zd, z) and same_bits(rd, r)
        assert same_bits(y, fast(r))
    finally:
        fast.close()


def test_upscale_on_a_strided_view_read_in_place():
    net = make_module(3, 1, "replicate", 7)
    fast = compile_module(net, input_range=2.0)
    calls = []
    inner = fast.ctx.process_f32_dev
    fast.ctx.process_f32_dev = lambda *a: (calls.append(a), inner(*a))[1]
    try:
        h, w = 19, 27
        x = torch.from_numpy(uniform((2, 3, h, w), 81))
        want = fast.upscale(x.cuda(), scale=2)
        big = torch.full((2, 6, h + 7, w + 21), GUARD)
        big[:, ::2, 3:3 + h, 10:10 + w] = x
        parent = big.cuda()
        view = parent[:, ::2, 3:3 + h, 10:10 + w]
        assert not view.is_contiguous()
        got = fast.upscale(view, scale=2)
        assert same_bits(got, want) and got.is_contiguous()
        assert calls[-1][0] == view.data_ptr() and calls[-1][1:6] == (w + 21, 2 * (h + 7) * (w + 21), 6 * (h + 7) * (w + 21), w, h)
        assert same_bits(fast.resize(view, (38, 54)), fast.resize(x.cuda(), (38, 54)))
        n_calls = len(calls)
        with pytest.raises(ValueError):
            fast.upscale(x.cuda().permute(0, 1, 3, 2), scale=2)          # innermost dimension not contiguous
        with pytest.raises(ValueError):
            fast.upscale(x, scale=2)                                     # a CPU tensor
        assert len(calls) == n_calls
    finally:
        fast.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_invalid_arguments_leave_the_context_usable(rctx):
    sh, sw, dh, dw = 17, 33, 25, 49
    x = torch.from_numpy(uniform((1, 2, sh, sw), 91)).cuda()
    want = resize_dev(rctx, x, dh, dw)
    out = torch.zeros((1, 2, dh, dw), device="cuda")
    big = torch.zeros(4 * dh * dw, device="cuda")
    torch.cuda.synchronize()
    p, q, sp, dp = x.data_ptr(), out.data_ptr(), sh * sw, dh * dw
    r = rctx.resize_cubic_f32_dev
    for bad in (lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, 0, dh, 2, 1),                # size 0
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, -3, 2, 1),
                lambda: r(p, sw, sp, 0, 0, sh, q, dw, dp, 0, dw, dh, 2, 1),
                lambda: r(p, sw - 1, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 2, 1),           # stride below the width
                lambda: r(p, sw, sp, 0, sw, sh, q, dw - 1, dp, 0, dw, dh, 2, 1),
                lambda: r(0, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 2, 1),               # null pointers
                lambda: r(p, sw, sp, 0, sw, sh, 0, dw, dp, 0, dw, dh, 2, 1),
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 0, 1),               # no channels, no frames
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 2, 0),
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp // 2, 0, dw, dh, 2, 1),          # output planes overlap each other
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 1, 2),               # two frames written to one place
                lambda: r(big.data_ptr(), sw, sp, 0, sw, sh, big.data_ptr() + 4 * sp, dw, dp, 0, dw, dh, 2, 1)):   # output over input
        assert "resize_cubic_f32_dev" in _err(bad, S.ERR_INVALID)
        assert same_bits(resize_dev(rctx, x, dh, dw), want), "a successful call on the same context after the refusal"
    host = x[0].cpu().numpy()
    with pytest.raises(S.SrcnnError):
        rctx._check(rctx._lib.srcnn_resize_cubic_f32(rctx._h, None, sw, sp, sw, sh, S._fp(np.empty((2, dh, dw), np.float32)), dw, dp,
                                                     dw, dh, 2))
    assert same_bits(rctx.resize_cubic_f32(host, dw, dh), want[0])
    assert rctx._lib.srcnn_abi_version() == 1


def test_process_gates_and_resize_in_every_mode(weights_blob):
    sh, sw, dh, dw = 20, 24, 40, 48
    x = torch.from_numpy(uniform((1, 1, sh, sw), 95)).cuda()
    with S.Context(0) as ctx:
        free = resize_dev(ctx, x, dh, dw)                                    # no model at all: the resize runs
        _err(lambda: process_dev(ctx, x, dh, dw), S.ERR_STATE)
        # layers loaded per filter (on a context that holds no whole model yet): refused, and named
        from srcnn_cpp_amd.synth import synth_luma
        w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
        y = synth_luma(96, 40)
        planes = [np.empty(y.shape, np.float32) for _ in range(32)]
        ctx.conv99x11(y, planes, w1, b1, w2, b2)
        ctx.conv55(planes, np.empty_like(y), w3, b3)
        msg = _err(lambda: process_dev(ctx, x, dh, dw), S.ERR_STATE)
        assert "per-filter" in msg, msg
        assert same_bits(resize_dev(ctx, x, dh, dw), free)
        ctx.set_weights_blob(weights_blob)                                   # a whole model: the call runs
        want = process_dev(ctx, x, dh, dw)
        assert same_bits(want, forward_dev(ctx, free))
        ctx.set_mode(S.MODE_EXACT)
        msg = _err(lambda: process_dev(ctx, x, dh, dw), S.ERR_STATE)
        assert f"mode {S.MODE_EXACT}" in msg, msg
        _err(lambda: ctx.process_f32(x[0, 0].cpu().numpy(), dw, dh), S.ERR_STATE)
        assert same_bits(resize_dev(ctx, x, dh, dw), free), "the resize runs in SRCNN_MODE_EXACT"
        ctx.set_mode(S.MODE_MFMA)
        assert same_bits(process_dev(ctx, x, dh, dw), want), "and the context runs the call again once the mode allows it"
        # a bad argument to process: SRCNN_ERR_INVALID, then a good call
        q = torch.zeros((1, 1, dh, dw), device="cuda")
        torch.cuda.synchronize()
        assert "process_f32_dev" in _err(lambda: ctx.process_f32_dev(x.data_ptr(), sw - 1, 0, 0, sw, sh, q.data_ptr(), dw, 0, 0, dw, dh, 1),
                                         S.ERR_INVALID)
        assert "process_f32_dev" in _err(lambda: ctx.process_f32_dev(x.data_ptr(), sw, 0, 0, sw, sh, q.data_ptr(), dw, 0, 0, dw, 0, 1),
                                         S.ERR_INVALID)
        assert same_bits(process_dev(ctx, x, dh, dw), want)
