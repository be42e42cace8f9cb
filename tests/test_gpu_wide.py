"""Models of other widths on the GPU (srcnn_set_model_shape: up to 128 / 64 filters; the wide forms of srcnn_spatial_kernels.hip): float64 references
at the tile edges of all three layers, three bitwise links to the 64 / 32 path (zero-embedded models, one-hot hidden channels,
integer-valued input through both paths), the band seams of a 1024 x 768 plane, batches with padded strides and guard
elements, a 128 / 64 nn.Module through compile_module, the narrow models, the refusals and model replacement.

Tolerance against float64: pre_tolerance(ref) * max(n1p / 64, n2p / 32).  pre_tolerance is the project's bound for the 64 / 32
kernels; float32 summation error is bounded linearly in the number of terms, and the longest sum of a padded model is n1p / 64
(layer 2) or n2p / 32 (layer 3) times as long."""
import copy

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from srcnn_cpp_amd.torch_api import compile_module
from color_reference import synth_color
from spatial_reference import assert_u8_consistent, pre_tolerance
from wide_reference import as_plain, band_seams, embed, forward, forward_rows, padded_widths, random_wide_model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 3), (9, 5), (17, 4), (130, 67), (260, 75)]          # the tile edges of all three layers
PADDINGS = ["replicate", "zero"]
OTHER_MODES = [S.MODE_EXACT, S.MODE_SPLIT16, S.MODE_REFBYTES, S.MODE_REFBYTES16, S.MODE_BANDED16]


@pytest.fixture(scope="module")
def wctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(wctx):
    def reset():
        wctx.set_mode(S.MODE_MFMA)
        wctx.set_padding("replicate")
    reset()
    yield
    reset()


def tolerance(ref, n1, n2):
    n1p, n2p = padded_widths(n1, n2)
    return pre_tolerance(ref) * max(n1p // 64, n2p // 32)


def byte_planes(channels, w, h, frame=0):
    """[C, h, w] uint8: the 8-bit test images."""
    x = synth_color(w, h, frame=frame) if channels == 3 else synth_luma(w, h, frame=frame)[:, :, None]
    return np.ascontiguousarray(np.moveaxis(x, 2, 0))


def float_planes(channels, w, h, frame=0):
    """[C, h, w] float32 in [0, 255] with non-integer values: the test images plus a quarter-step dither."""
    x = byte_planes(channels, w, h, frame).astype(np.float32)
    d = np.float32(0.25) * ((np.arange(w)[None] + np.arange(h)[:, None]) % 4).astype(np.float32) - np.float32(0.375)
    return np.clip(x + d[None], 0, 255).astype(np.float32)


def run_f32(ctx, x):
    return ctx.forward_f32(x[0])[None] if x.shape[0] == 1 else ctx.forward_f32(x)


def run_u8(ctx, x):
    """The byte path on [C, h, w] uint8 planes: (out [C, h, w] uint8, pre-clamp [C, h, w] float32)."""
    if x.shape[0] == 1:
        pre = np.empty(x.shape[1:], np.float32)
        return ctx.forward_y(x[0], preclamp=pre)[None], pre[None]
    img = np.ascontiguousarray(np.moveaxis(x, 0, 2))
    pre = np.empty(img.shape, np.float32)
    out = ctx.forward_color(img, preclamp=pre)
    return np.ascontiguousarray(np.moveaxis(out, 2, 0)), np.ascontiguousarray(np.moveaxis(pre, 2, 0))


def check_against_float64(ctx, model, channels, n1, n2, padding, sizes, what):
    """Both paths of the loaded model on every size; returns the largest error / tolerance seen."""
    worst = (0.0, 0.0)
    for w, h in sizes:
        xb, xf = byte_planes(channels, w, h, frame=2), float_planes(channels, w, h, frame=3)
        ref = forward(xb, model, padding)
        assert np.abs(ref).max() < 2000          # the model does not saturate: the test sees real values
        tol = tolerance(ref, n1, n2)
        out, pre = run_u8(ctx, xb)
        err = np.abs(pre.astype(np.float64) - ref).max()
        assert err <= tol, f"{what} {w}x{h} bytes: error {err:.3g}, tolerance {tol:.3g}"
        assert_u8_consistent(out, ref, tol)
        worst = max(worst, (err / tol, err))
        ref = forward(xf, model, padding)
        tol = tolerance(ref, n1, n2)
        got = run_f32(ctx, xf)
        assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref).max()
        assert err <= tol, f"{what} {w}x{h} floats: error {err:.3g}, tolerance {tol:.3g}"
        worst = max(worst, (err / tol, err))
    print(f"{what}: largest error {worst[1]:.3g} ({worst[0]:.3f} of the tolerance)")


# ---- 1: against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_128_64_matches_float64(wctx, channels, f2, padding):
    model = random_wide_model(channels, 128, f2, 64, 1)
    wctx.set_model(*model)
    wctx.set_padding(padding)
    assert wctx.model_shape() == (channels, 128, f2, 64) and wctx.model_channels() == channels and wctx.model_f2() == f2
    check_against_float64(wctx, model, channels, 128, 64, padding, SIZES, f"128/64 {channels}ch 9-{f2}-5 {padding}")


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n1,n2", [(128, 32), (64, 64), (96, 48), (100, 40)])
def test_other_widths_match_float64(wctx, n1, n2, channels, padding):
    model = random_wide_model(channels, n1, 3, n2, 2)
    wctx.set_model(*model)
    wctx.set_padding(padding)
    assert wctx.model_shape() == (channels, n1, 3, n2)
    check_against_float64(wctx, model, channels, n1, n2, padding, [(130, 67)], f"{n1}/{n2} {channels}ch 9-3-5 {padding}")


# ---- 2: a 64 / 32 model embedded in 128 / 64 tensors gives the floats of the 64 / 32 path ---------------------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_zero_embedded_64_32_model_is_bitwise_the_existing_path(wctx, channels, f2, padding):
    """The real channels first, zeros after: every term the padding adds is an exact 0, so the summation orders of the wide
    kernels are the existing ones continued if and only if the floats are equal (+0 equals -0)."""
    model = random_wide_model(channels, 64, f2, 32, 3)
    for w, h in [(130, 67), (260, 75)]:
        x = float_planes(channels, w, h, frame=f2)
        wctx.set_model(*as_plain(model))
        wctx.set_padding(padding)
        assert wctx.model_shape() == (channels, 64, f2, 32)
        want = run_f32(wctx, x)
        for n1, n2 in [(128, 64), (128, 32), (64, 64)]:
            wctx.set_model(*embed(model, n1, n2))
            assert wctx.model_shape() == (channels, n1, f2, n2)
            got = run_f32(wctx, x)
            assert np.array_equal(got, want), (w, h, n1, n2, np.abs(got - want).max())
        assert len(np.unique(want)) > h


# ---- 3: one-hot hidden channels: any group or chunk offset error shows exactly --------------------------------------------
def one_hot_model(channels, f2, k1, k2):
    """A 128 / 64 model whose only non-zero hidden channels are k1 (layer 1) and k2 (layer 2), with the same values whatever
    (k1, k2) is; positive weights, so that the channels are alive."""
    w1, b1, w2, b2, w3, b3 = random_wide_model(channels, 128, f2, 64, 4)
    W1, B1, W2, B2, W3 = (np.zeros_like(a) for a in (w1, b1, w2, b2, w3))
    W1[k1], B1[k1] = np.abs(w1[5]), np.abs(b1[5])
    W2[k2, k1], B2[k2] = np.abs(w2[3, 5]), np.abs(b2[3])
    W3[:, k2] = w3[:, 3] * 8
    return W1, B1, W2, B2, W3, b3


@pytest.mark.parametrize("k1,k2", [(127, 63), (64, 32), (65, 33), (63, 31)])
@pytest.mark.parametrize("channels,f2,padding", [(1, 1, "replicate"), (1, 3, "zero"), (1, 5, "replicate"), (3, 1, "zero"),
                                                 (3, 3, "replicate"), (3, 5, "zero")])
def test_one_hot_channels_equal_the_pair_moved_to_0_0(wctx, channels, f2, padding, k1, k2):
    x = float_planes(channels, 130, 67, frame=1)
    wctx.set_padding(padding)
    wctx.set_model(*one_hot_model(channels, f2, 0, 0))
    want = run_f32(wctx, x)
    assert len(np.unique(want)) > 67, "the hidden channels are alive"
    wctx.set_model(*one_hot_model(channels, f2, k1, k2))
    got = run_f32(wctx, x)
    assert np.array_equal(got, want), np.abs(got - want).max()
    ref = forward(x, one_hot_model(channels, f2, k1, k2), padding)
    assert np.abs(got - ref).max() <= tolerance(ref, 128, 64)


# ---- 4: on integer-valued input the byte path's pre-clamp floats are the float path's output ------------------------------
@pytest.mark.parametrize("n1,n2,channels,padding", [(128, 64, c, p) for c in (1, 3) for p in PADDINGS] +
                         [(128, 32, 1, "zero"), (128, 32, 3, "replicate"), (128, 32, 3, "zero"), (64, 64, 1, "replicate")])
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_bitwise_equal_to_the_byte_paths_preclamp(wctx, n1, n2, channels, padding, f2):
    """Wherever layer 3 runs a wide form (n2p = 64) or spatial_l3_kernel (n2p = 32, but for bytes of 1 channel
    under replicate padding, which MODE_L3 runs): the same arithmetic in the same order on both paths."""
    wctx.set_model(*random_wide_model(channels, n1, f2, n2, 5))
    wctx.set_padding(padding)
    for w, h in [(1, 1), (17, 4), (130, 67), (260, 75)]:
        xb = byte_planes(channels, w, h, frame=f2)
        _, pre = run_u8(wctx, xb)
        got = run_f32(wctx, xb.astype(np.float32))
        assert np.array_equal(got.view(np.uint32), pre.view(np.uint32)), (w, h, np.abs(got - pre).max())


# ---- 5: band seams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f2,channels,padding", [(3, 1, "replicate"), (3, 3, "zero"), (5, 1, "zero"), (5, 3, "replicate")])
def test_1024x768_row_windows_across_the_band_seam(wctx, f2, channels, padding):
    """768 B per pixel of a 1024 x 768 plane exceed the 512 MiB of the band maps: two bands.  Every window's reference comes
    from only the input rows it needs, so only true image edges are padded."""
    w, h = 1024, 768
    model = random_wide_model(channels, 128, f2, 64, 6)
    wctx.set_model(*model)
    wctx.set_padding(padding)
    seams = band_seams(w, h, f2, 128, 64)
    assert seams == [384]
    xb, xf = byte_planes(channels, w, h, frame=4), float_planes(channels, w, h, frame=5)
    windows = [(0, 12), (h - 12, h)] + [(s - 8, s + 8) for s in seams]
    out, pre = run_u8(wctx, xb)
    got = run_f32(wctx, xf)
    for r0, r1 in windows:
        ref = forward_rows(xb, model, r0, r1, padding)
        tol = tolerance(ref, 128, 64)
        assert np.abs(pre[:, r0:r1].astype(np.float64) - ref).max() <= tol, (r0, r1)
        assert_u8_consistent(out[:, r0:r1], ref, tol)
        ref = forward_rows(xf, model, r0, r1, padding)
        err = np.abs(got[:, r0:r1].astype(np.float64) - ref).max()
        assert err <= tolerance(ref, 128, 64), f"rows {r0}..{r1}: error {err:.3g}"


# ---- 6: batches, padded strides and pitches, guard elements ---------------------------------------------------------------
def test_luma_device_batch_with_pitches_and_guards(wctx):
    model = random_wide_model(1, 128, 3, 64, 7)
    wctx.set_model(*model)
    w, h, n = 203, 37, 3
    sstride, dstride = 256, 224
    spitch, dpitch = sstride * h + 96, dstride * h + 32
    frames = np.stack([synth_luma(w, h, frame=k) for k in range(n)])
    src = torch.zeros(n * spitch, dtype=torch.uint8)
    for k in range(n):
        src[k * spitch:k * spitch + sstride * h].view(h, sstride)[:, :w] = torch.from_numpy(frames[k])
    d_src = src.cuda()
    d_dst = torch.full((n * dpitch,), 0xA5, dtype=torch.uint8, device="cuda")
    d_pre = torch.full((n * dpitch,), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    wctx.forward_y_dev(d_src.data_ptr(), sstride, spitch, d_dst.data_ptr(), dstride, dpitch, w, h, n, d_pre.data_ptr())
    wctx.synchronize()
    dst, pre = d_dst.cpu().numpy(), d_pre.cpu().numpy()
    written = np.zeros(n * dpitch, bool)
    for k in range(n):
        want_out, want_pre = run_u8(wctx, frames[k][None])
        view = lambda a: a[k * dpitch:k * dpitch + dstride * h].reshape(h, dstride)[:, :w]
        assert np.array_equal(view(dst), want_out[0]) and np.array_equal(view(pre), want_pre[0])
        view(written)[:] = True
    assert (dst[~written] == 0xA5).all() and (pre[~written] == -7.5).all(), "guard bytes and floats stay intact"
    assert np.array_equal(wctx.forward_y_frames(frames), np.stack([run_u8(wctx, f[None])[0][0] for f in frames]))
    ref = forward(frames[1][None], model)
    assert_u8_consistent(run_u8(wctx, frames[1][None])[0], ref, tolerance(ref, 128, 64))


def test_colour_device_batch_with_pitches_and_guards(wctx):
    model = random_wide_model(3, 128, 5, 64, 8)
    wctx.set_model(*model)
    wctx.set_padding("zero")
    w, h, n = 131, 21, 3
    sstride, dstride = 3 * w + 11, 3 * w + 5
    spitch, dpitch = sstride * h + 64, dstride * h + 16
    imgs = [synth_color(w, h, frame=k) for k in range(n)]
    src = torch.zeros(n * spitch, dtype=torch.uint8)
    for k in range(n):
        src[k * spitch:k * spitch + sstride * h].view(h, sstride)[:, :3 * w] = torch.from_numpy(imgs[k].reshape(h, 3 * w))
    d_src = src.cuda()
    d_dst = torch.full((n * dpitch,), 0x5A, dtype=torch.uint8, device="cuda")
    d_pre = torch.full((n * dpitch,), -3.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    wctx.forward_color_dev(d_src.data_ptr(), sstride, spitch, d_dst.data_ptr(), dstride, dpitch, w, h, n, d_pre.data_ptr())
    wctx.synchronize()
    dst, pre = d_dst.cpu().numpy(), d_pre.cpu().numpy()
    written = np.zeros(n * dpitch, bool)
    for k in range(n):
        want_pre = np.empty(imgs[k].shape, np.float32)
        want_out = wctx.forward_color(imgs[k], preclamp=want_pre)
        view = lambda a: a[k * dpitch:k * dpitch + dstride * h].reshape(h, dstride)[:, :3 * w]
        assert np.array_equal(view(dst), want_out.reshape(h, 3 * w)) and np.array_equal(view(pre), want_pre.reshape(h, 3 * w))
        view(written)[:] = True
    assert (dst[~written] == 0x5A).all() and (pre[~written] == -3.25).all(), "guard bytes and floats stay intact"


@pytest.mark.parametrize("channels", [1, 3])
def test_float_device_batch_with_pitches_and_guards(wctx, channels):
    model = random_wide_model(channels, 128, 3, 64, 9)
    wctx.set_model(*model)
    w, h, n = 131, 23, 3
    sstride, dstride = w + 5, w + 3
    sch, dch = sstride * h + 7, dstride * h + 9
    sfr, dfr = channels * sch + 13, channels * dch + 11
    frames = [float_planes(channels, w, h, frame=k) for k in range(n)]
    src = torch.zeros(n * sfr, dtype=torch.float32)
    for k in range(n):
        for c in range(channels):
            o = k * sfr + c * sch
            src[o:o + sstride * h].view(h, sstride)[:, :w] = torch.from_numpy(frames[k][c])
    d_src = src.cuda()
    d_dst = torch.full((n * dfr,), -9.75, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    wctx.forward_f32_dev(d_src.data_ptr(), sstride, sch, sfr, d_dst.data_ptr(), dstride, dch, dfr, w, h, n)
    wctx.synchronize()
    dst = d_dst.cpu().numpy()
    written = np.zeros(n * dfr, bool)
    for k in range(n):
        want = run_f32(wctx, frames[k])
        for c in range(channels):
            o = k * dfr + c * dch
            assert np.array_equal(dst[o:o + dstride * h].reshape(h, dstride)[:, :w], want[c])
            written[o:o + dstride * h].reshape(h, dstride)[:, :w] = True
    assert (dst[~written] == -9.75).all(), "guard floats stay intact"


def test_process_bgr_equals_the_composed_steps(wctx):
    wctx.set_model(*random_wide_model(1, 128, 3, 64, 10))
    bgr = (np.random.default_rng(3).integers(0, 256, (41, 53, 3)) // 8 * 8).astype(np.uint8)
    ow, oh = S.scaled_size(53, 41, 2.0)
    planes = [wctx.resize_cubic(p, ow, oh) for p in wctx.bgr2ycrcb(bgr)]
    want = wctx.ycrcb2bgr(wctx.forward_y(planes[0]), planes[1], planes[2])
    assert np.array_equal(wctx.process_bgr(bgr, 2.0), want)
    wctx.set_model(*random_wide_model(3, 128, 3, 64, 10))
    up = np.stack([wctx.resize_cubic(np.ascontiguousarray(bgr[:, :, c]), ow, oh) for c in range(3)], axis=2)
    assert np.array_equal(wctx.process_bgr(bgr, 2.0), wctx.forward_color(np.ascontiguousarray(up)))


# ---- 7: a 128 / 64 nn.Module through compile_module -----------------------------------------------------------------------
class WideSRCNN(torch.nn.Module):
    def __init__(self, channels, f2, padding_mode):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(channels, 128, 9, padding=4, padding_mode=padding_mode)
        self.conv2 = torch.nn.Conv2d(128, 64, f2, padding=f2 // 2, padding_mode=padding_mode)
        self.conv3 = torch.nn.Conv2d(64, channels, 5, padding=2, padding_mode=padding_mode)

    def forward(self, x):
        return self.conv3(torch.relu(self.conv2(torch.relu(self.conv1(x)))))


def wide_module(channels, f2, padding_mode, seed):
    torch.manual_seed(seed)
    net = WideSRCNN(channels, f2, padding_mode)
    with torch.no_grad():
        net.conv3.bias.add_(0.4)
    return net.eval()


def module64(net, x):
    with torch.no_grad():
        return copy.deepcopy(net).double()(torch.as_tensor(np.asarray(x)).double()).numpy()


def unit_tolerance(ref):
    """The tolerance for [0, 1] data: that of 0..255 data, carried over by homogeneity, for 128 / 64 filters."""
    return tolerance(np.asarray(ref) * 255.0, 128, 64) / 255.0


@pytest.mark.parametrize("channels,f2,padding_mode", [(1, 3, "zeros"), (3, 5, "replicate")])
def test_module_batch_of_two_on_a_side_stream_and_upscale(channels, f2, padding_mode):
    net = wide_module(channels, f2, padding_mode, 5)
    fast = compile_module(net, device=0)
    try:
        assert fast.ctx.model_shape() == (channels, 128, f2, 64)
        x = torch.from_numpy(np.stack([float_planes(channels, 97, 61, frame=k) / np.float32(255.0) for k in range(2)]))
        side = torch.cuda.Stream()
        d_x = x.cuda()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = fast(d_x)
        side.synchronize()
        assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda
        ref = module64(net, x)
        err = np.abs(got.cpu().numpy() - ref).max()
        assert err <= unit_tolerance(ref), f"error {err:.3g}, tolerance {unit_tolerance(ref):.3g}"
        # upscale(x, scale=2) is the module on the library's own bicubic resize (tests/test_gpu_resize_f32.py holds that resize
        # to F.interpolate): the float64 module on the same resized tensor, so that only the model's arithmetic error enters
        lr = d_x[:, :, :30, :48].contiguous()
        up = fast.resize(lr, (60, 96))
        z = fast.upscale(lr, scale=2)
        assert z.shape == (2, channels, 60, 96)
        assert torch.equal(z, fast(up))
        ref = module64(net, up.cpu())
        assert np.abs(z.cpu().numpy() - ref).max() <= unit_tolerance(ref)
    finally:
        fast.close()


def test_module_upscale_rgb_image_on_stored_uint8_pixels():
    """An H x W x 3 uint8 picture through upscale_rgb_image of a 128 / 64 luma module, against the script it replaces with the
    module itself in float64 (the bound of tests/test_gpu_image.py: 0.5 for the store's rounding plus 255 times the float
    path's tolerance and the resize's)."""
    from resize_f32_reference import TOL
    from rgb_f32_reference import BT601_FULL, classic64, luma_lr_f32
    net = wide_module(1, 3, "zeros", 6)
    fast = compile_module(net, device=0)
    try:
        sh, sw, dh, dw = 30, 61, 60, 122
        hwc = np.random.default_rng(11).integers(0, 256, (sh, sw, 3)).astype(np.uint8)
        x = np.ascontiguousarray(np.moveaxis(hwc, 2, 0)).astype(np.float32) * np.float32(1.0 / 255.0)
        conv, luma = BT601_FULL, BT601_FULL.luma()
        got = fast.upscale_rgb_image(torch.from_numpy(hwc).cuda().permute(2, 0, 1), scale=2, luma=luma)
        assert got.dtype == torch.uint8 and got.shape == (3, dh, dw) and got.stride() == (1, dw * 3, 3)
        yup = fast.resize(torch.from_numpy(luma_lr_f32(x, luma)[None, None]).cuda(), (dh, dw))[0, 0].cpu().numpy()
        model64 = lambda y: module64(net, np.asarray(y)[None, None])[0, 0]
        ref = classic64(x, dh, dw, conv, model64, yup=yup)
        g = S.luma_gain(luma)
        tol = g * unit_tolerance(model64(yup.astype(np.float64))) + 2 * TOL * (float(np.abs(x).max()) + g * float(np.abs(yup).max()))
        err = np.abs(got.cpu().numpy().astype(np.float64) - np.clip(ref * 255.0, 0.0, 255.0))
        print(f"upscale_rgb_image: max |got - clip(ref * 255)| = {err.max():.4f}, bound {0.5 + 255 * tol:.4f}")
        assert (err <= 0.5 + 255.0 * tol).all()
    finally:
        fast.close()


# ---- 8: a narrow model is an ordinary model -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [S.MODE_MFMA, S.MODE_REFBYTES])
def test_narrow_32_16_is_set_weights_on_the_padded_tensors(wctx, mode):
    model = random_wide_model(1, 32, 1, 16, 11)
    padded = as_plain(embed(model, 64, 32))
    y = synth_luma(300, 170, frame=2)
    wctx.set_weights(*padded)
    wctx.set_mode(mode)
    want = wctx.forward_y(y)
    wctx.set_model(*model)
    assert wctx.model_shape() == (1, 32, 1, 16)
    assert np.array_equal(wctx.forward_y(y), want)
    ref = forward(y[None], model)[0]
    assert_u8_consistent(want, ref, pre_tolerance(ref))
    wctx.set_weights(*padded)
    assert wctx.model_shape() == (1, 64, 1, 32)


@pytest.mark.parametrize("channels,f2", [(1, 3), (3, 1), (3, 5)])
def test_narrow_models_of_the_other_loaders(wctx, channels, f2):
    model = random_wide_model(channels, 32, f2, 16, 12)
    x = byte_planes(channels, 130, 67, frame=1)
    wctx.set_model(*as_plain(embed(model, 64, 32)))
    want = run_u8(wctx, x)
    wctx.set_model(*model)
    assert wctx.model_shape() == (channels, 32, f2, 16)
    got = run_u8(wctx, x)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    wctx.set_mode(S.MODE_BANDED16)              # every mode that runs such a model runs this one
    run_u8(wctx, x)


# ---- 9: refusals and model replacement ------------------------------------------------------------------------------------
def _state(fn):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == S.ERR_STATE
    return str(e.value)


def test_refused_modes_and_entry_points_leave_the_context_usable(wctx):
    model = random_wide_model(1, 128, 3, 64, 13)
    wctx.set_model(*model)
    w, h = 64, 32
    y = synth_luma(w, h)
    before = wctx.forward_y(y)
    d_src = torch.from_numpy(y).cuda()
    d_dst = torch.zeros_like(d_src)
    d_work = torch.zeros(32 * w * h, dtype=torch.float32, device="cuda")
    d_f = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    d_g = torch.zeros(w * h, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p, o = d_src.data_ptr(), d_dst.data_ptr()
    calls = [lambda: wctx.forward_y_rows_dev(p, w, 0, o, w, 0, w, h, 0, h),
             lambda: wctx.forward_y_rows_halo_dev(p, w, 0, h, 0, 0, w, o, w, 0, w, h, 0, h),
             lambda: wctx.forward_y_unfused_dev(p, w, 0, o, w, 0, w, h, 1, d_work.data_ptr()),
             lambda: wctx.conv99x11_dev(p, w, d_work.data_ptr(), w, w * h, w, h),
             lambda: wctx.conv55_dev(d_work.data_ptr(), w, w * h, o, w, w, h),
             lambda: S.forward_y_striped([wctx], y),
             lambda: S.forward_y_striped_frames([wctx], y[None]),
             lambda: S.forward_y_frames_multi([wctx], y[None]),
             lambda: S.forward_y_lanes_dev([wctx], [p], w, [o], w, w, h),
             lambda: S.forward_y_striped_dev([wctx], [p], w, [o], w, w, h),
             lambda: wctx.model_rows_dev(p, w, 0, o, w, 0, w, h, 0, h),
             lambda: wctx.model_rows_halo_dev(p, w, 0, h, 0, 0, w, o, w, 0, w, h, 0, h),
             lambda: wctx.model_rows_f32_dev(d_f.data_ptr(), w, 0, 0, d_g.data_ptr(), w, 0, 0, w, h, 0, h),
             lambda: S.model_striped([wctx], y),
             lambda: S.model_striped_dev([wctx], [p], w, [o], w, w, h),
             lambda: S.model_striped_f32([wctx], y.astype(np.float32))]
    for k, call in enumerate(calls):
        msg = _state(call)
        assert "128" in msg and "64" in msg, (k, msg)
    for mode in OTHER_MODES:
        wctx.set_mode(mode)
        for call in (lambda: wctx.forward_y(y), lambda: wctx.forward_y_frames(y[None]), lambda: wctx.forward_f32(y.astype(np.float32)),
                     lambda: wctx.forward_y_dev(p, w, 0, o, w, 0, w, h, 1)):
            msg = _state(call)
            assert "128" in msg and "64" in msg and "SRCNN_MODE_MFMA" in msg, (mode, msg)
    wctx.set_mode(S.MODE_MFMA)
    assert wctx.model_shape() == (1, 128, 3, 64)
    assert np.array_equal(wctx.forward_y(y), before)          # the model is still there and runs
    # a colour wide model: its stripes, and the 1-channel entry points
    wctx.set_model(*random_wide_model(3, 100, 3, 40, 13))
    img = synth_color(w, h)
    d_img = torch.from_numpy(img).cuda()
    d_out = torch.zeros_like(d_img)
    torch.cuda.synchronize()
    for call in (lambda: wctx.model_color_rows_dev(d_img.data_ptr(), 3 * w, 0, d_out.data_ptr(), 3 * w, 0, w, h, 0, h),
                 lambda: S.model_color_striped([wctx], img), lambda: wctx.forward_y(y)):
        msg = _state(call)
        assert "100" in msg and "40" in msg, msg
    wctx.forward_color(img)


def test_bad_shapes_are_invalid_and_keep_the_loaded_model(wctx):
    model = random_wide_model(1, 128, 3, 64, 14)
    wctx.set_model(*model)
    y = synth_luma(70, 30, frame=4)
    before = wctx.forward_y(y)
    z = np.zeros(128 * 128 * 25, np.float32)
    fp = lambda a: a.ctypes.data_as(S._f32p)
    for channels, n1, f2, n2 in [(1, 129, 3, 64), (1, 128, 3, 65), (1, 0, 3, 64), (1, 128, 3, 0), (2, 128, 3, 64), (1, 128, 7, 64),
                                 (1, 128, 2, 64), (4, 64, 1, 32), (1, -1, 1, 32)]:
        rc = wctx._lib.srcnn_set_model_shape(wctx._h, channels, n1, f2, n2, fp(z), fp(z), fp(z), fp(z), fp(z), fp(z))
        assert rc == S.ERR_INVALID, (channels, n1, f2, n2)
    assert wctx._lib.srcnn_set_model_shape(wctx._h, 1, 128, 3, 64, fp(z), fp(z), None, fp(z), fp(z), fp(z)) == S.ERR_INVALID
    assert wctx.model_shape() == (1, 128, 3, 64)
    assert np.array_equal(wctx.forward_y(y), before)


def test_model_replacement(wctx, weights_blob):
    """After a wide model the default 9-1-5 weights give the bytes a fresh context gives; srcnn_set_model and
    srcnn_set_model_color replace it as well, and a per-filter call that loads weights ends it."""
    y = synth_luma(300, 170, frame=1)
    fresh = S.Context(0)
    try:
        fresh.set_weights_blob(weights_blob)
        want = {mode: (fresh.set_mode(mode), fresh.forward_y(y))[1] for mode in (S.MODE_MFMA, S.MODE_REFBYTES)}
    finally:
        fresh.close()
    for mode in (S.MODE_MFMA, S.MODE_REFBYTES):
        wctx.set_mode(S.MODE_MFMA)
        wctx.set_model(*random_wide_model(1, 128, 1, 64, 15))
        wctx.forward_y(y)
        wctx.set_weights_blob(weights_blob)
        assert wctx.model_shape() == (1, 64, 1, 32)
        wctx.set_mode(mode)
        assert np.array_equal(wctx.forward_y(y), want[mode])
    wctx.set_mode(S.MODE_MFMA)
    # srcnn_set_model / srcnn_set_model_color after a wide model: the result of a context that never held one
    for channels in (1, 3):
        plain = as_plain(random_wide_model(channels, 64, 3, 32, 16))
        x = byte_planes(channels, 130, 67)
        wctx.set_weights_blob(weights_blob)
        wctx.set_model(*plain)
        want_u8 = run_u8(wctx, x)
        wctx.set_model(*random_wide_model(4 - channels, 128, 5, 64, 16))
        wctx.set_model(*plain)
        assert wctx.model_shape() == (channels, 64, 3, 32)
        got = run_u8(wctx, x)
        assert np.array_equal(got[0], want_u8[0]) and np.array_equal(got[1], want_u8[1])
    # a per-filter call that loads weights ends the wide model
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    wctx.set_model(*random_wide_model(1, 128, 1, 64, 17))
    small = synth_luma(70, 30)
    wctx.conv55([np.ones(small.shape, np.float32)] * 32, np.empty(small.shape, np.uint8), w3, b3)
    assert wctx.model_shape() == (1, 64, 1, 32)
    _state(lambda: wctx.forward_y(small))
    wctx.set_model(*random_wide_model(1, 128, 1, 64, 17))
    wctx.forward_y(small)
