"""A 3-plane float image through a 1-channel model on the GPU (srcnn_process_rgb_f32(_dev), CompiledModule.upscale_rgb): bit for
bit the composition of existing calls and float32 numpy, the program it replaces in float64 and with torch's own resize,
layouts, the torch front end on both kinds of stream, refusals.  All planes are small."""
import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.torch_api import compile_module
from color_reference import random_color_model
from resize_f32_reference import TOL, torch_cpu
from rgb_f32_reference import BT601_FULL, BT601_STUDIO, SAME_SHAPES, SHAPES, classic64, luma_lr_f32, merge_f32, rgb
from spatial_reference import random_model, torch_forward
from test_gpu_f32 import scaled_tolerance
from zero_pad_reference import torch_forward_zero

pytestmark = pytest.mark.gpu

GUARD = float("nan")
# (f2, padding, mode): random 1-channel models at both layer-2 sizes, both paddings, both modes
CONFIGS = [(f2, padding, mode) for f2 in (1, 5) for padding in ("replicate", "zero") for mode in (S.MODE_MFMA, S.MODE_BANDED16)]
LUMAS = [BT601_FULL.luma(), BT601_STUDIO.luma(), S.luma_for_order(S.LUMA_BT601, "bgr")]
CLAMP = (0.0, 1.0)
MODEL_SEED = 3


def load(ctx, f2, padding, mode):
    ctx.set_model(*random_model(f2, MODEL_SEED))
    ctx.set_padding(padding)
    ctx.set_mode(mode)
    ctx.set_input_range(1.0)          # [0, 1] data


@pytest.fixture(scope="module")
def ctxs():
    """One context per model configuration, made when first asked for and shared by the tests of this file."""
    made = {}

    def get(config):
        if config not in made:
            made[config] = S.Context(0)
            load(made[config], *config)
        return made[config]
    yield get
    for c in made.values():
        c.close()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rgb_dev(ctx, x, dh, dw, luma, clamp=None):
    """srcnn_process_rgb_f32_dev on a contiguous CUDA tensor (N, 3, H, W), on the context's stream."""
    n, c, h, w = x.shape
    assert c == 3 and x.is_contiguous() and x.dtype == torch.float32
    out = torch.full((n, 3, dh, dw), GUARD, dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()
    ctx.process_rgb_f32_dev(x.data_ptr(), w, h * w, 3 * h * w, w, h, out.data_ptr(), dw, dh * dw, 3 * dh * dw, dw, dh, luma, clamp, n)
    ctx.synchronize()
    return out


def resize_dev(ctx, x, dh, dw):
    n, c, h, w = x.shape
    out = torch.full((n, c, dh, dw), GUARD, dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()
    ctx.resize_cubic_f32_dev(x.data_ptr(), w, h * w, c * h * w, w, h, out.data_ptr(), dw, dh * dw, c * dh * dw, dw, dh, c, n)
    ctx.synchronize()
    return out


def forward_dev(ctx, y):
    """The loaded 1-channel model on a contiguous CUDA plane (H, W)."""
    h, w = y.shape
    out = torch.full_like(y, GUARD)
    torch.cuda.synchronize()
    ctx.forward_f32_dev(y.data_ptr(), w, 0, 0, out.data_ptr(), w, 0, 0, w, h, 1)
    ctx.synchronize()
    return out


def composed(ctx, x, dh, dw, luma):
    """The pieces of the call from existing calls, as float32 numpy: U (3, dh, dw), Yup, Ysr (dh, dw) and the library's g."""
    u = resize_dev(ctx, dev(x)[None], dh, dw)[0].cpu().numpy()
    yup = resize_dev(ctx, dev(luma_lr_f32(x, luma))[None, None], dh, dw)[0, 0]
    ysr = forward_dev(ctx, yup.contiguous()).cpu().numpy()
    return u, yup.cpu().numpy(), ysr, np.float32(S.luma_gain(luma))


# ---- 1: bit for bit the composition of existing calls ----------------------------------------------------------------------
@pytest.mark.parametrize("case", list(enumerate(SHAPES + SAME_SHAPES)), ids=lambda c: "x".join(map(str, c[1])))
def test_bitwise_equal_to_the_composition_at_every_shape(ctxs, case):
    k, (sh, sw, dh, dw) = case
    ctx, luma = ctxs(CONFIGS[k % len(CONFIGS)]), LUMAS[k % len(LUMAS)]
    x = rgb((3, sh, sw), 100 + k)
    u, yup, ysr, g = composed(ctx, x, dh, dw, luma)
    assert np.isfinite(ysr).all()
    free = rgb_dev(ctx, dev(x)[None], dh, dw, luma)[0].cpu().numpy()
    assert same_bits(free, merge_f32(u, ysr, yup, g))
    bound = rgb_dev(ctx, dev(x)[None], dh, dw, luma, CLAMP)[0].cpu().numpy()
    assert same_bits(bound, merge_f32(u, ysr, yup, g, CLAMP))
    assert bound.min() >= 0.0 and bound.max() <= 1.0
    if dh * dw >= 100:
        assert free.min() < 0.0 or free.max() > 1.0, "the result overshoots [0, 1]: the clamp has something to bind"
        assert not same_bits(free, bound)
    if (sh, sw) == (dh, dw):
        # no resize: U is x and Yup is Y, so numpy alone states the result around the model
        y = luma_lr_f32(x, luma)
        assert same_bits(u, x) and same_bits(yup, y)
        assert same_bits(free, x + ((forward_dev(ctx, dev(y)).cpu().numpy() - y) * g)[None])


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"9-{c[0]}-5-{c[1]}-mode{c[2]}")
def test_bitwise_equal_to_the_composition_for_every_model(ctxs, config):
    ctx = ctxs(config)
    for k, (sh, sw, dh, dw) in enumerate([(17, 33, 25, 49), (12, 100, 20, 257)]):
        luma = LUMAS[k]
        x = rgb((3, sh, sw), 200 + k)
        u, yup, ysr, g = composed(ctx, x, dh, dw, luma)
        assert same_bits(rgb_dev(ctx, dev(x)[None], dh, dw, luma)[0], merge_f32(u, ysr, yup, g))
        assert same_bits(rgb_dev(ctx, dev(x)[None], dh, dw, luma, CLAMP)[0], merge_f32(u, ysr, yup, g, CLAMP))


# ---- 2: the program the call replaces, in float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("conv", [BT601_FULL, BT601_STUDIO], ids=lambda c: c.name)
@pytest.mark.parametrize("config", [CONFIGS[k] for k in (0, 3, 5, 6)], ids=lambda c: f"9-{c[0]}-5-{c[1]}-mode{c[2]}")
@pytest.mark.parametrize("sh,sw,dh,dw", [(17, 33, 25, 49), (30, 120, 45, 260)])
def test_against_the_classic_round_trip_in_float64(ctxs, conv, config, sh, sw, dh, dw):
    """The round trip through the full matrix and its exact inverse, the model in float64 on the GPU's own Yup (so only the
    model's arithmetic error enters, not its sensitivity to input rounding).  Tolerance: the model's, times g, plus
    2 TOL (max|x| + g max|Y|) for the two resizes and the 7 roundings of steps 1 and 4 beside the 12 TOL counts.  Then the same
    script with torch's own F.interpolate, within that plus torch's drift, computed from the two references alone."""
    f2, padding, _ = config
    ctx, luma = ctxs(config), conv.luma()
    model = random_model(f2, MODEL_SEED)
    model64 = (lambda y: torch_forward(y, model)) if padding == "replicate" else (lambda y: torch_forward_zero(y, model))
    x = rgb((3, sh, sw), 300 + sh)
    yup = resize_dev(ctx, dev(luma_lr_f32(x, luma))[None, None], dh, dw)[0, 0].cpu().numpy()
    got = rgb_dev(ctx, dev(x)[None], dh, dw, luma)[0].cpu().numpy().astype(np.float64)
    ref = classic64(x, dh, dw, conv, model64, yup=yup)
    g = S.luma_gain(luma)
    ysr_ref = model64(yup.astype(np.float64))
    tol = g * scaled_tolerance(ysr_ref, 1.0) + 2 * TOL * (float(np.abs(x).max()) + g * float(np.abs(yup).max()))
    err = np.abs(got - ref).max()
    tor = classic64(x, dh, dw, conv, model64, yup=yup, resize=torch_cpu)
    drift = np.abs(tor - ref).max()
    err_t = np.abs(got - tor).max()
    print(f"{conv.name} {config} {sh}x{sw} -> {dh}x{dw}: |got - classic64| = {err:.3g} (tol {tol:.3g}), with torch's resize "
          f"{err_t:.3g} (tol + {drift:.3g})")
    assert err <= tol
    assert err_t <= tol + drift


# ---- 3: layouts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_off,dst_pad", [(1, 9), (4, 12), (3, 8)])
@pytest.mark.parametrize("sh,sw,dh,dw", [(17, 33, 25, 49), (20, 130, 40, 260)])
def test_strided_views_in_guarded_tensors(ctxs, sh, sw, dh, dw, dst_off, dst_pad):
    """Source and destination as windows of larger NaN-filled tensors at odd element offsets, with row, channel and frame
    strides of their own: (4, 12) on 260 columns aligns every destination row (vector stores), the odd pitches change the
    alignment from row to row, (3, 8) on 260 columns aligns none.  Same bits as contiguous tensors, guards untouched."""
    ctx, luma, n = ctxs(CONFIGS[2]), LUMAS[1], 2
    x = torch.from_numpy(rgb((n, 3, sh, sw), 31))
    want = rgb_dev(ctx, x.cuda(), dh, dw, luma, CLAMP)
    src_parent = torch.full((n, 4, sh + 5, sw + 7), GUARD)
    src_parent[:, :3, 2:2 + sh, 3:3 + sw] = x
    src_parent = src_parent.cuda()
    src = src_parent[:, :3, 2:2 + sh, 3:3 + sw]
    dst_parent = torch.full((n, 5, dh + 3, dw + dst_pad), GUARD, device="cuda")
    dst = dst_parent[:, 1:4, 1:1 + dh, dst_off:dst_off + dw]
    torch.cuda.synchronize()
    ctx.process_rgb_f32_dev(src.data_ptr(), src.stride(2), src.stride(1), src.stride(0), sw, sh,
                            dst.data_ptr(), dst.stride(2), dst.stride(1), dst.stride(0), dw, dh, luma, CLAMP, n)
    ctx.synchronize()
    assert same_bits(dst.contiguous(), want)
    outside = torch.ones_like(dst_parent, dtype=torch.bool)
    outside[:, 1:4, 1:1 + dh, dst_off:dst_off + dw] = False
    assert torch.isnan(dst_parent[outside]).all(), "the floats around the destination window stay untouched"
    assert torch.isnan(src_parent[:, 3]).all()


def test_three_frames_equal_three_single_calls(ctxs):
    ctx, luma = ctxs(CONFIGS[5]), LUMAS[0]
    sh, sw, dh, dw = 12, 100, 20, 257
    x = dev(rgb((3, 3, sh, sw), 41))
    got = rgb_dev(ctx, x, dh, dw, luma)
    assert torch.isfinite(got).all()
    for f in range(3):
        assert same_bits(got[f], rgb_dev(ctx, x[f:f + 1].contiguous(), dh, dw, luma)[0]), f


def test_host_form_equals_device_form(ctxs):
    ctx, luma = ctxs(CONFIGS[0]), LUMAS[1]
    sh, sw, dh, dw = 17, 33, 25, 49
    x = rgb((3, sh, sw), 51)
    for clamp in (None, CLAMP):
        want = rgb_dev(ctx, dev(x)[None], dh, dw, luma, clamp)[0].cpu().numpy()
        assert same_bits(ctx.process_rgb_f32(x, dw, dh, luma, clamp), want)
        wide = np.full((3, sh + 2, sw + 5), np.float32(GUARD))
        wide[:, 1:1 + sh, 2:2 + sw] = x
        assert same_bits(ctx.process_rgb_f32(wide[:, 1:1 + sh, 2:2 + sw], dw, dh, luma, clamp), want)     # a strided host view
    assert same_bits(ctx.process_rgb_f32(x, dw, dh), rgb_dev(ctx, dev(x)[None], dh, dw, S.LUMA_BT601)[0])   # the default luma


@pytest.mark.parametrize("config", [CONFIGS[0], CONFIGS[7]], ids=lambda c: f"9-{c[0]}-5-{c[1]}-mode{c[2]}")
def test_workspace_regrowth_matches_fresh_contexts(config):
    """One context running a small call and then a larger one -- the second grows the two-plane workspace -- and the small one
    again, against a fresh context per shape."""
    shapes = [(17, 33, 25, 49), (20, 24, 40, 48), (17, 33, 25, 49)]
    xs = [dev(rgb((2, 3, sh, sw), 60 + sh)) for sh, sw, _, _ in shapes]
    with S.Context(0) as ctx:
        load(ctx, *config)
        seq = [rgb_dev(ctx, x, dh, dw, LUMAS[0], CLAMP) for x, (_, _, dh, dw) in zip(xs, shapes)]
    assert same_bits(seq[0], seq[2])
    for x, got, (_, _, dh, dw) in zip(xs[:2], seq, shapes):
        with S.Context(0) as fresh:
            load(fresh, *config)
            assert same_bits(rgb_dev(fresh, x, dh, dw, LUMAS[0], CLAMP), got)


# ---- 4: the torch front end ------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("padding_mode,mode", [("zeros", S.MODE_MFMA), ("replicate", S.MODE_BANDED16)])
def test_upscale_rgb_batch_scale_size_and_the_context_call(padding_mode, mode):
    fast = compile_module(make_module(1, 3, padding_mode, 5), mode=mode, input_range=2.0)
    try:
        luma = S.luma_bt601_studio(1.0)
        x = dev(rgb((3, 3, 21, 30), 71))                                   # a batch of 3
        by_scale = fast.upscale_rgb(x, scale=2, luma=luma, clamp=CLAMP)
        assert by_scale.shape == (3, 3, 42, 60) and by_scale.dtype == torch.float32 and by_scale.device == x.device
        assert same_bits(by_scale, fast.upscale_rgb(x, size=(42, 60), luma=luma, clamp=CLAMP))
        assert same_bits(by_scale, rgb_dev(fast.ctx, x, 42, 60, luma, CLAMP)), "the Context's device call, bit for bit"
        assert fast.upscale_rgb(x, scale=1.5).shape == (3, 3, 31, 45)          # (int)(21 * 1.5), (int)(30 * 1.5)
        one = fast.upscale_rgb(x[1], scale=2, luma=luma, clamp=CLAMP)          # (3, H, W) in, (3, H', W') out
        assert one.shape == (3, 42, 60) and same_bits(one, by_scale[1])
        # the pieces through the same front end: resize of the planes, the module on the resized luma
        free = fast.upscale_rgb(x[:1], size=(31, 47), luma=luma)
        xn = x[0].cpu().numpy()
        y = fast.upscale(dev(luma_lr_f32(xn, luma))[None, None], size=(31, 47))[0, 0].cpu().numpy()
        ctx3 = fast.ctx.resize_cubic_f32_dev
        u = torch.empty((1, 3, 31, 47), device="cuda")
        yup = torch.empty((1, 1, 31, 47), device="cuda")
        yl = dev(luma_lr_f32(xn, luma))
        torch.cuda.synchronize()
        ctx3(x.data_ptr(), 30, 21 * 30, 0, 30, 21, u.data_ptr(), 47, 31 * 47, 0, 47, 31, 3, 1)
        ctx3(yl.data_ptr(), 30, 0, 0, 30, 21, yup.data_ptr(), 47, 0, 0, 47, 31, 1, 1)
        fast.ctx.synchronize()
        assert same_bits(free[0], merge_f32(u[0].cpu().numpy(), y, yup[0, 0].cpu().numpy(), np.float32(S.luma_gain(luma))))
        same = fast.upscale_rgb(x, size=(21, 30))                               # no resize
        assert same.shape == x.shape and not same_bits(same, x)
    finally:
        fast.close()


def test_upscale_rgb_on_a_non_default_stream_and_on_the_default_stream():
    fast = compile_module(make_module(1, 1, "zeros", 6), input_range=2.0)
    try:
        x = dev(rgb((2, 3, 40, 52), 81))
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            y = fast.upscale_rgb(x, scale=2)
            z = y * 2.0 + 1.0                         # the next torch op on that stream consumes the result unsynchronised
        stream.synchronize()
        assert same_bits(z, y * 2.0 + 1.0), "the op queued behind the call saw the finished result"
        yd = fast.upscale_rgb(x * 1.0, scale=2)       # the default stream, interleaved with torch's own work on it
        zd = yd * 2.0 + 1.0
        torch.cuda.synchronize()
        assert same_bits(yd, y) and same_bits(zd, z)
    finally:
        fast.close()


def test_upscale_rgb_on_a_channel_strided_view_read_in_place():
    fast = compile_module(make_module(1, 1, "replicate", 7), input_range=2.0)
    calls = []
    inner = fast.ctx.process_rgb_f32_dev
    fast.ctx.process_rgb_f32_dev = lambda *a: (calls.append(a), inner(*a))[1]
    try:
        h, w = 19, 27
        x = torch.from_numpy(rgb((2, 3, h, w), 91))
        want = fast.upscale_rgb(x.cuda(), scale=2)
        big = torch.full((2, 6, h + 7, w + 21), GUARD)
        big[:, ::2, 3:3 + h, 10:10 + w] = x
        parent = big.cuda()
        view = parent[:, ::2, 3:3 + h, 10:10 + w]
        assert not view.is_contiguous()
        got = fast.upscale_rgb(view, scale=2)
        assert same_bits(got, want) and got.is_contiguous()
        assert calls[-1][0] == view.data_ptr() and calls[-1][1:6] == (w + 21, 2 * (h + 7) * (w + 21), 6 * (h + 7) * (w + 21), w, h)
        n_calls = len(calls)
        with pytest.raises(ValueError):
            fast.upscale_rgb(x.cuda().permute(0, 1, 3, 2), scale=2)          # innermost dimension not contiguous
        with pytest.raises(ValueError):
            fast.upscale_rgb(x.cuda(), size=(h - 1, w))                      # shrinks
        with pytest.raises(ValueError):
            fast.upscale_rgb(x.cuda(), scale=2, luma=(0.0, 0.0, 0.0, 0.0))
        with pytest.raises(ValueError):
            fast.upscale_rgb(x.cuda(), scale=2, clamp=(1.0, 0.0))
        assert len(calls) == n_calls
    finally:
        fast.close()


# ---- 5: refusals -----------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_state_refusals_leave_the_context_usable():
    sh, sw, dh, dw = 17, 33, 25, 49
    x = dev(rgb((1, 3, sh, sw), 95))
    luma = LUMAS[0]
    with S.Context(0) as ctx:
        _err(lambda: rgb_dev(ctx, x, dh, dw, luma), S.ERR_STATE)                              # no model
        _err(lambda: ctx.process_rgb_f32(x[0].cpu().numpy(), dw, dh), S.ERR_STATE)
        ctx.set_model(*random_color_model(1, 3))                                              # a 3-channel model
        msg = _err(lambda: rgb_dev(ctx, x, dh, dw, luma), S.ERR_STATE)
        assert "srcnn_process_f32" in msg, msg
        load(ctx, 1, "zero", S.MODE_MFMA)
        want = rgb_dev(ctx, x, dh, dw, luma)
        assert torch.isfinite(want).all()
        for mode in (S.MODE_EXACT, S.MODE_SPLIT16):
            ctx.set_mode(mode)
            msg = _err(lambda: rgb_dev(ctx, x, dh, dw, luma), S.ERR_STATE)
            assert f"mode {mode}" in msg, msg
            _err(lambda: ctx.process_rgb_f32(x[0].cpu().numpy(), dw, dh), S.ERR_STATE)
            ctx.set_mode(S.MODE_MFMA)
            assert same_bits(rgb_dev(ctx, x, dh, dw, luma), want), "the context runs the call again once the mode allows it"


def test_invalid_arguments_leave_the_context_usable(ctxs):
    ctx, luma = ctxs(CONFIGS[4]), LUMAS[0]
    sh, sw, dh, dw = 23, 29, 31, 37
    x = dev(rgb((1, 3, sh, sw), 97))
    want = rgb_dev(ctx, x, dh, dw, luma, CLAMP)
    out = torch.zeros((1, 3, dh, dw), device="cuda")
    big = torch.zeros(8 * dh * dw, device="cuda")
    torch.cuda.synchronize()
    p, q, sp, dp = x.data_ptr(), out.data_ptr(), sh * sw, dh * dw
    lib, h = ctx._lib, ctx._h
    import ctypes as C
    l4 = (C.c_float * 4)(*luma)

    def raw(src=p, sstride=sw, spitch=sp, w=sw, hh=sh, dst=q, dstride=dw, dpitch=dp, ow=dw, oh=dh, lu=l4, clamp=None, n=1, fp=0):
        c2 = None if clamp is None else (C.c_float * 2)(*clamp)
        return lambda: ctx._check(lib.srcnn_process_rgb_f32_dev(h, src, sstride, spitch, 0, w, hh, dst, dstride, dpitch, fp, ow, oh, lu, c2, n))

    nan, inf = float("nan"), float("inf")
    for bad in (raw(ow=13, oh=11),                                   # the issue's shrinking size (23, 29) -> (11, 13)
                raw(ow=sw - 1), raw(oh=sh - 1),                      # one axis shrinks
                raw(ow=0), raw(oh=-3), raw(w=0),                     # sizes
                raw(sstride=sw - 1), raw(dstride=dw - 1),            # stride below the width
                raw(src=None), raw(dst=None), raw(n=0),
                raw(dpitch=dp // 2),                                 # output planes overlap each other
                raw(n=2),                                            # two frames written to one place
                raw(src=big.data_ptr(), dst=big.data_ptr() + 4 * sp),                    # output over input
                raw(src=big.data_ptr(), dst=big.data_ptr()),                             # aliased
                raw(lu=None), raw(lu=(C.c_float * 4)(nan, 0.5, 0.5, 0.0)), raw(lu=(C.c_float * 4)(0.3, 0.6, 0.1, inf)),
                raw(lu=(C.c_float * 4)(0.0, 0.0, 0.0, 0.0)), raw(lu=(C.c_float * 4)(0.5, -0.25, -0.25, 0.0)),
                raw(clamp=(1.0, 0.0)), raw(clamp=(nan, 1.0)), raw(clamp=(0.0, nan))):
        assert "process_rgb_f32_dev" in _err(bad, S.ERR_INVALID)
        assert same_bits(rgb_dev(ctx, x, dh, dw, luma, CLAMP), want), "a successful call on the same context after the refusal"
    assert not torch.isnan(out).any() and float(out.abs().max()) == 0.0, "a refused call wrote nothing"
    host = np.empty((3, dh, dw), np.float32)
    assert lib.srcnn_process_rgb_f32(h, S._fp(x[0].cpu().numpy()), sw, sp, sw, sh, S._fp(host), dw, dp, 13, 11, l4, None) == S.ERR_INVALID
    assert lib.srcnn_process_rgb_f32(h, None, sw, sp, sw, sh, S._fp(host), dw, dp, dw, dh, l4, None) == S.ERR_INVALID
    assert same_bits(ctx.process_rgb_f32(x[0].cpu().numpy(), dw, dh, luma, CLAMP), want[0])
    assert lib.srcnn_abi_version() == 1
