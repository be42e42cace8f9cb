"""Colour SRCNN models (srcnn_set_model_color) on the GPU: float64 references for both paddings, 4K row windows across the band
seams, an exact one-hot channel-routing check, a real 3-channel nn.Module, the device form, process_bgr, the refusals, ending
the model, and two contexts."""
import numpy as np
import pytest
import torch

import oracle
import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from spatial_reference import assert_u8_consistent, band_seams, pre_tolerance, random_model, torch_forward
from color_reference import random_color_model, synth_color, torch_forward_color, torch_forward_color_rows

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 3), (9, 5), (17, 4), (130, 67), (260, 75), (1920, 1080)]
OTHER_MODES = [S.MODE_EXACT, S.MODE_SPLIT16, S.MODE_REFBYTES, S.MODE_REFBYTES16]
PADDINGS = ["replicate", "zero"]


@pytest.fixture(scope="module")
def cctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _mfma(cctx):
    cctx.set_mode(S.MODE_MFMA)
    cctx.set_padding("replicate")
    yield
    cctx.set_mode(S.MODE_MFMA)
    cctx.set_padding("replicate")


def run(ctx, img):
    pre = np.empty(img.shape, np.float32)
    out = ctx.forward_color(img, preclamp=pre)
    return out, pre


def check(out, pre, ref):
    tol = pre_tolerance(ref)
    assert np.abs(pre.astype(np.float64) - ref).max() <= tol
    assert_u8_consistent(out, ref, tol)


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_matches_float64(cctx, f2, padding):
    model = random_color_model(f2, 1)
    cctx.set_padding(padding)
    cctx.set_model(*model)
    assert cctx.model_channels() == 3 and cctx.model_f2() == f2
    for w, h in SIZES:
        img = synth_color(w, h, frame=f2)
        out, pre = run(cctx, img)
        ref = torch_forward_color(img, model, padding)
        assert np.abs(ref).max() < 2000
        check(out, pre, ref)


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 5])
def test_3840x2160_row_windows_across_band_seams(cctx, f2, padding):
    model = random_color_model(f2, 2)
    cctx.set_padding(padding)
    cctx.set_model(*model)
    w, h = 3840, 2160
    img = synth_color(w, h, frame=3)
    out, pre = run(cctx, img)
    seams = band_seams(w, h, f2)
    assert seams
    for r0, r1 in [(0, 12), (h - 12, h)] + [(s - 8, s + 8) for s in seams]:
        ref = torch_forward_color_rows(img, model, r0, r1, padding)
        check(out[r0:r1], pre[r0:r1], ref)


def one_hot_model(f2):
    """Output channel c copies input channel PERM[c] shifted by SHIFT[c] (an asymmetric layer-1 tap), in integers: layer 1 puts
    the tapped input channel c' on map channel c' (weight 1), layer 2 passes map channel c' to channel c' (centre tap 1),
    layer 3 takes map channel PERM[c] for output c (centre tap 1).  Every value stays an integer below 256."""
    w1 = np.zeros((64, 3, 9, 9), np.float32)
    for c in range(3):
        dy, dx = SHIFT[c]
        w1[PERM[c], PERM[c], 4 + dy, 4 + dx] = 1.0
    w2 = np.zeros((32, 64, f2, f2), np.float32)
    for k in range(3):
        w2[k, k, f2 // 2, f2 // 2] = 1.0
    w3 = np.zeros((3, 32, 5, 5), np.float32)
    for c in range(3):
        w3[c, PERM[c], 2, 2] = 1.0
    return w1, np.zeros(64, np.float32), w2, np.zeros(32, np.float32), w3, np.zeros(3, np.float32)


PERM = [2, 0, 1]
SHIFT = [(-3, 2), (1, -4), (4, 3)]     # (dy, dx) of the layer-1 tap of output channel c, on input channel PERM[c]


def shifted(plane, dy, dx, padding):
    """out[y, x] = plane[y + dy, x + dx], replicate- or zero-padded."""
    h, w = plane.shape
    p = np.pad(plane, 4, mode="edge" if padding == "replicate" else "constant")
    return p[4 + dy:4 + dy + h, 4 + dx:4 + dx + w]


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_exact_channel_routing(cctx, f2, padding):
    """A permuting, shifting one-hot model in integer arithmetic: bytes must match exactly (interleave, channel order, tap
    orientation and the borders), which a tolerance would hide."""
    # (with the shifted plane 1 / 1-layer-2-and-3 taps being centred, the layer-1 tap alone sets the shift; the border is the
    # first layer's padding: replicate repeats the edge pixel, zero brings 0)
    cctx.set_padding(padding)
    cctx.set_model(*one_hot_model(f2))
    for w, h in [(37, 23), (300, 140)]:
        img = synth_color(w, h, frame=7)
        want = np.stack([shifted(img[:, :, PERM[c]], *SHIFT[c], padding) for c in range(3)], axis=2)
        out, pre = run(cctx, img)
        assert np.array_equal(out, want)
        assert np.array_equal(pre, want.astype(np.float32))


class ColorSRCNN(torch.nn.Module):
    def __init__(self, f2):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 64, 9, padding=4)
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=f2 // 2)
        self.conv3 = torch.nn.Conv2d(32, 3, 5, padding=2)

    def forward(self, x):
        return self.conv3(torch.relu(self.conv2(torch.relu(self.conv1(x)))))


def test_pytorch_module_end_to_end(cctx):
    """A 3-channel nn.Module trained on RGB in [0, 1] runs on a BGR image: model_from_module(image_order="bgr")."""
    torch.manual_seed(5)
    net = ColorSRCNN(5).double()
    with torch.no_grad():
        net.conv3.bias.add_(0.4)
    model, padding = S.model_from_module(net, image_order="bgr")
    assert padding == "zero"
    cctx.set_padding(padding)
    cctx.set_model(*model)
    bgr = synth_color(97, 61, frame=2)
    rgb = bgr[:, :, ::-1]
    with torch.no_grad():
        ref_rgb = net(torch.from_numpy(np.ascontiguousarray(np.moveaxis(rgb, 2, 0), dtype=np.float64))[None] / 255.0)[0].numpy()
    ref = np.moveaxis(ref_rgb * 255.0, 0, 2)[:, :, ::-1]       # the module's output, back in BGR order, on 0..255
    assert np.abs(ref).max() < 2000
    check(*run(cctx, bgr), ref)


def test_device_frames_strides_and_preclamp(cctx):
    model = random_color_model(3, 3)
    cctx.set_padding("zero")
    cctx.set_model(*model)
    w, h, n = 133, 47, 3
    ss, sp = 3 * w + 29, (3 * w + 29) * h + 77          # padded strides and frame pitches, in bytes
    ds, dp = 3 * w + 16, (3 * w + 16) * h + 40
    imgs = [synth_color(w, h, frame=10 + k) for k in range(n)]
    src = np.zeros(sp * n, np.uint8)
    for k, im in enumerate(imgs):
        for y in range(h):
            src[k * sp + y * ss:k * sp + y * ss + 3 * w] = im[y].ravel()
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.zeros(dp * n, dtype=torch.uint8, device="cuda")
    d_pre = torch.zeros(dp * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    cctx.forward_color_dev(d_src.data_ptr(), ss, sp, d_dst.data_ptr(), ds, dp, w, h, n, d_pre.data_ptr())
    cctx.synchronize()
    dst, pre = d_dst.cpu().numpy(), d_pre.cpu().numpy()
    for k, im in enumerate(imgs):
        rows = lambda a: np.stack([a[k * dp + y * ds:k * dp + y * ds + 3 * w] for y in range(h)]).reshape(h, w, 3)
        check(rows(dst), rows(pre), torch_forward_color(im, model, "zero"))
    # the bytes between rows and frames stay untouched
    mask = np.ones(dp * n, bool)
    for k in range(n):
        for y in range(h):
            mask[k * dp + y * ds:k * dp + y * ds + 3 * w] = False
    assert not dst[mask].any() and not pre[mask].any()


@pytest.mark.parametrize("padding", PADDINGS)
def test_process_bgr_with_a_colour_model(cctx, padding):
    model = random_color_model(1, 4)
    cctx.set_padding(padding)
    cctx.set_model(*model)
    bgr = synth_color(71, 45, frame=4)
    scale = 2.0
    out = cctx.process_bgr(bgr, scale)
    ow, oh = S.scaled_size(71, 45, scale)
    up = np.stack([oracle.resize_cubic(np.ascontiguousarray(bgr[:, :, c]), ow, oh) for c in range(3)], axis=2)
    assert np.array_equal(np.stack([cctx.resize_cubic(np.ascontiguousarray(bgr[:, :, c]), ow, oh) for c in range(3)], axis=2), up)
    ref = torch_forward_color(up, model, padding)
    tol = pre_tolerance(ref)
    assert_u8_consistent(out, ref, tol)
    # the device form gives the same bytes
    d_bgr = torch.from_numpy(bgr.copy()).cuda()
    d_out = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cctx.process_bgr_dev(d_bgr.data_ptr(), 3 * 71, 71, 45, scale, d_out.data_ptr(), 3 * ow)
    cctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), out)


def _state(fn):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == S.ERR_STATE
    return str(e.value)


@pytest.mark.parametrize("padding", PADDINGS)
def test_refusals_with_a_colour_model(cctx, weights_blob, padding):
    """A replicate colour 9-1-5 model passes every test of f2 and padding: the luma entry points must still refuse it."""
    model = random_color_model(1, 5)
    cctx.set_padding(padding)
    cctx.set_model(*model)
    w, h = 64, 32
    y = synth_luma(w, h)
    d_src = torch.from_numpy(y).cuda()
    d_dst = torch.zeros_like(d_src)
    d_work = torch.zeros(32 * w * h, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p, o = d_src.data_ptr(), d_dst.data_ptr()
    msgs = [
        _state(lambda: cctx.forward_y(y)),
        _state(lambda: cctx.forward_y(y, preclamp=np.empty(y.shape, np.float32))),
        _state(lambda: cctx.forward_y_frames(np.stack([y, y]))),
        _state(lambda: cctx.forward_y_dev(p, w, 0, o, w, 0, w, h, 1)),
        _state(lambda: cctx.forward_y_rows_dev(p, w, 0, o, w, 0, w, h, 0, h)),
        _state(lambda: cctx.forward_y_rows_halo_dev(p, w, 0, h, 0, 0, w, o, w, 0, w, h, 0, h)),
        _state(lambda: cctx.forward_y_unfused_dev(p, w, 0, o, w, 0, w, h, 1, d_work.data_ptr())),
        _state(lambda: cctx.conv99x11_dev(p, w, d_work.data_ptr(), w, w * h, w, h)),
        _state(lambda: cctx.conv55_dev(d_work.data_ptr(), w, w * h, o, w, w, h)),
        _state(lambda: S.forward_y_striped([cctx], y)),
        _state(lambda: S.forward_y_striped_frames([cctx], y[None])),
        _state(lambda: S.forward_y_frames_multi([cctx], y[None])),
        _state(lambda: S.forward_y_lanes_dev([cctx], [p], w, [o], w, w, h)),
        _state(lambda: S.forward_y_striped_dev([cctx], [p], w, [o], w, w, h)),
    ]
    assert all("colour" in m for m in msgs), msgs
    assert cctx.model_channels() == 3 and cctx.model_f2() == 1
    img = synth_color(40, 24, frame=1)
    for mode in OTHER_MODES:
        cctx.set_mode(mode)
        assert "SRCNN_MODE_MFMA" in _state(lambda: cctx.forward_color(img))
        _state(lambda: cctx.forward_y(y))
        _state(lambda: cctx.process_bgr(img, 2.0))
    cctx.set_mode(S.MODE_MFMA)
    check(*run(cctx, img), torch_forward_color(img, model, padding))      # the context still runs the model
    # a 1-channel model: forward_color refuses
    cctx.set_weights_blob(weights_blob)
    assert cctx.model_channels() == 1
    assert "1-channel" in _state(lambda: cctx.forward_color(img))
    d_img = torch.from_numpy(img).cuda()
    d_out = torch.zeros_like(d_img)
    torch.cuda.synchronize()
    _state(lambda: cctx.forward_color_dev(d_img.data_ptr(), 120, 0, d_out.data_ptr(), 120, 0, 40, 24, 1))


def test_ending_the_model(cctx, weights_blob):
    y = synth_luma(300, 170, frame=2)
    img = synth_color(50, 30)
    fresh = S.Context(0)
    try:
        fresh.set_weights_blob(weights_blob)
        for mode in [S.MODE_MFMA] + OTHER_MODES:
            cctx.set_mode(S.MODE_MFMA)
            cctx.set_model(*random_color_model(3, 6))
            cctx.set_weights_blob(weights_blob)
            assert cctx.model_channels() == 1 and cctx.model_f2() == 1
            cctx.set_mode(mode)
            fresh.set_mode(mode)
            assert np.array_equal(cctx.forward_y(y), fresh.forward_y(y)), mode
    finally:
        fresh.close()
    cctx.set_mode(S.MODE_MFMA)
    luma = random_model(5, 7)
    cctx.set_model(*luma)
    before = cctx.forward_y(y)
    cctx.set_model(*random_color_model(5, 7))
    run(cctx, img)
    cctx.set_model(*luma)
    assert cctx.model_channels() == 1
    assert np.array_equal(cctx.forward_y(y), before)
    # a per-filter call that loads weights ends a colour model as well
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    cctx.set_model(*random_color_model(1, 8))
    cctx.conv99x11(y, [np.empty(y.shape, np.float32) for _ in range(32)], w1, b1, w2, b2)
    assert cctx.model_channels() == 1 and cctx.model_f2() == 1
    _state(lambda: cctx.forward_color(img))


def test_two_contexts_keep_their_own_models(cctx):
    color, luma = random_color_model(3, 9), random_model(3, 9)
    other = S.Context(0)
    try:
        cctx.set_model(*color)
        other.set_model(*luma)
        img = synth_color(90, 50, frame=6)
        y = synth_luma(90, 50, frame=6)
        check(*run(cctx, img), torch_forward_color(img, color))
        pre = np.empty(y.shape, np.float32)
        other.forward_y(y, preclamp=pre)
        assert np.abs(pre - torch_forward(y, luma)).max() <= pre_tolerance(torch_forward(y, luma))
        assert cctx.model_channels() == 3 and other.model_channels() == 1
        _state(lambda: cctx.forward_y(y))
        _state(lambda: other.forward_color(img))
    finally:
        other.close()
