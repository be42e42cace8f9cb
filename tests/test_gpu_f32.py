"""The float image path on the GPU (srcnn_forward_f32, srcnn_forward_f32_dev, srcnn_set_input_range, torch_api.compile_module):
the bitwise link to the byte path's pre-clamp floats, float64 references for all twelve model configurations in both modes on
[0, 1] and 10-bit data, 4K row windows across the band seams, real nn.Modules through compile_module, the device form, the
refusals and the range setting."""
import copy

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from srcnn_cpp_amd.torch_api import compile_module
from color_reference import random_color_model, synth_color, torch_forward_color, torch_forward_color_rows
from spatial_reference import band_seams, pre_tolerance, random_model, torch_forward, torch_forward_rows
from zero_pad_reference import torch_forward_zero, torch_forward_zero_rows

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 3), (9, 5), (17, 4), (130, 67), (260, 75), (1920, 1080)]       # test_gpu_color.SIZES
MODES = [S.MODE_MFMA, S.MODE_BANDED16]
OTHER_MODES = [S.MODE_EXACT, S.MODE_SPLIT16, S.MODE_REFBYTES, S.MODE_REFBYTES16]
PADDINGS = ["replicate", "zero"]


@pytest.fixture(scope="module")
def fctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(fctx):
    def reset():
        fctx.set_mode(S.MODE_MFMA)
        fctx.set_padding("replicate")
        fctx.set_input_range(255.0)
    reset()
    yield
    reset()


def scaled_tolerance(ref, r):
    """The project's tolerance for 0..255 data, carried to data of range r by homogeneity."""
    return pre_tolerance(np.asarray(ref) * 255.0 / r) * r / 255.0


def make_model(channels, f2, seed):
    return random_color_model(f2, seed) if channels == 3 else random_model(f2, seed)


def unit_planes(channels, w, h, frame=0):
    """[C, h, w] float32 in [0, 1]: the 8-bit test images over 255 (non-integer values)."""
    x = synth_color(w, h, frame=frame) if channels == 3 else synth_luma(w, h, frame=frame)[:, :, None]
    return np.ascontiguousarray(np.moveaxis(x, 2, 0)).astype(np.float32) / np.float32(255.0)


def ten_bit_planes(channels, w, h, frame=0):
    """[C, h, w] float32 in [0, 1023] with non-integer values: the test images times 1023 / 255 plus a quarter-step dither."""
    x = unit_planes(channels, w, h, frame) * np.float32(1023.0)
    d = np.float32(0.25) * ((np.arange(w)[None] + np.arange(h)[:, None]) % 4).astype(np.float32) - np.float32(0.375)
    return np.clip(x + d[None], 0, 1023).astype(np.float32)


def reference(x, model, padding, rows=None):
    """float64 [C, h, w] (rows: [C, r1 - r0, w]) of the model on the planes x [C, h, w]."""
    if x.shape[0] == 3:
        img = np.moveaxis(x, 0, 2)
        ref = torch_forward_color(img, model, padding) if rows is None else torch_forward_color_rows(img, model, *rows, padding)
        return np.moveaxis(ref, 2, 0)
    if rows is None:
        return (torch_forward(x[0], model) if padding == "replicate" else torch_forward_zero(x[0], model))[None]
    return (torch_forward_rows(x[0], model, *rows) if padding == "replicate" else torch_forward_zero_rows(x[0], model, *rows))[None]


def run(ctx, x):
    """forward_f32 on [C, h, w] planes ((h, w) for one channel, to use that form of the binding too)."""
    if x.shape[0] == 1:
        return ctx.forward_f32(x[0])[None]
    return ctx.forward_f32(x)


def check(got, ref, r, what=""):
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.isfinite(got).all(), what
    err, tol = np.abs(got.astype(np.float64) - ref).max(), scaled_tolerance(ref, r)
    assert err <= tol, f"{what}: error {err:.3g}, tolerance {tol:.3g}"


# ---- 8: on integer-valued input the float planes ARE the byte path's pre-clamp floats -------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels,padding", [(1, "zero"), (3, "replicate"), (3, "zero")])
def test_bitwise_equal_to_the_byte_paths_preclamp(fctx, channels, padding, f2, mode):
    """Every configuration whose byte path runs spatial_l3_kernel: the same kernel arithmetic in the same order, so the float
    output equals the pre-clamp array bit for bit (the colour pre-clamp is interleaved, the float planes are not)."""
    fctx.set_model(*make_model(channels, f2, 1))
    fctx.set_padding(padding)
    fctx.set_mode(mode)
    for w, h in [(1, 1), (17, 4), (130, 67), (260, 75), (517, 301)]:
        if channels == 3:
            img = synth_color(w, h, frame=f2)
            pre = np.empty(img.shape, np.float32)
            fctx.forward_color(img, preclamp=pre)
            want = np.ascontiguousarray(np.moveaxis(pre, 2, 0))
            x = np.ascontiguousarray(np.moveaxis(img, 2, 0)).astype(np.float32)
        else:
            y = synth_luma(w, h, frame=f2)
            pre = np.empty(y.shape, np.float32)
            fctx.forward_y(y, preclamp=pre)
            want, x = pre[None], y.astype(np.float32)[None]
        got = run(fctx, x)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, h, np.abs(got - want).max())


# ---- 9: all twelve configurations against float64, both modes, [0, 1] and 10-bit data -------------------------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_matches_float64(fctx, channels, f2, padding):
    """A model as trained (biases not scaled) on synth / 255 with range 1, and on a 0..1023 plane with range 1023."""
    model = make_model(channels, f2, 1)
    fctx.set_model(*model)
    fctx.set_padding(padding)
    assert fctx.model_channels() == channels and fctx.model_f2() == f2
    for w, h in SIZES:
        for r, x in ((1.0, unit_planes(channels, w, h, frame=f2)), (1023.0, ten_bit_planes(channels, w, h, frame=f2))):
            assert np.abs(x).max() <= r
            ref = reference(x, model, padding)
            fctx.set_input_range(r)
            for mode in MODES:
                fctx.set_mode(mode)
                check(run(fctx, x), ref, r, f"{w}x{h} range {r} mode {mode}")


# ---- 10: 3840x2160 row windows across the band seams ----------------------------------------------------------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("channels", [1, 3])
def test_3840x2160_row_windows_across_band_seams(fctx, channels, padding):
    f2 = 5
    model = make_model(channels, f2, 2)
    fctx.set_model(*model)
    fctx.set_padding(padding)
    fctx.set_input_range(1.0)
    w, h = 3840, 2160
    x = unit_planes(channels, w, h, frame=3)
    seams = band_seams(w, h, f2)
    assert seams
    windows = [(0, 12), (h - 12, h)] + [(s - 8, s + 8) for s in seams]
    refs = [reference(x, model, padding, rows=win) for win in windows]
    for mode in MODES:
        fctx.set_mode(mode)
        got = run(fctx, x)
        for (r0, r1), ref in zip(windows, refs):
            check(got[:, r0:r1], ref, 1.0, f"rows {r0}..{r1} mode {mode}")


# ---- 11: real nn.Modules through compile_module ---------------------------------------------------------------------------
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
    net = SRCNN(channels, f2, padding_mode)
    with torch.no_grad():
        net.conv3.bias.add_(0.4)
    return net.eval()


def module_reference(net, x):
    with torch.no_grad():
        return copy.deepcopy(net).double()(x.detach().cpu().double()).numpy()


def batch(channels, n, w, h):
    return torch.from_numpy(np.stack([unit_planes(channels, w, h, frame=k) for k in range(n)]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("padding_mode", ["zeros", "replicate"])
@pytest.mark.parametrize("channels", [1, 3])
def test_module_batch_of_three(channels, padding_mode, mode):
    net = make_module(channels, 5 if channels == 1 else 3, padding_mode, 5)
    fast = compile_module(net, device=0, mode=mode, input_range=1.0)
    try:
        assert fast.ctx.padding() == ("zero" if padding_mode == "zeros" else "replicate")
        x = batch(channels, 3, 97, 61)
        got = fast(x.cuda())
        assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda
        check(got.cpu().numpy(), module_reference(net, x), 1.0)
        one = fast(x[1].cuda())                               # (C, H, W) in, (C, H, W) out, the same values as in the batch
        assert one.shape == x.shape[1:]
        assert torch.equal(one, got[1])
    finally:
        fast.close()


@pytest.mark.parametrize("channels,padding_mode,mode", [(3, "zeros", S.MODE_MFMA), (1, "replicate", S.MODE_MFMA),
                                                        (3, "replicate", S.MODE_BANDED16), (1, "zeros", S.MODE_BANDED16)])
def test_module_on_strided_views_read_in_place(channels, padding_mode, mode):
    """Channel- and row-strided views go to the library with data_ptr() and their strides.  That no copy is made is checked on
    the call the callable makes: the source address is the view's own, the strides are the view's, and the floats of the
    parent tensor outside the view are never read (they hold NaN, which would spread into the result)."""
    net = make_module(channels, 3, padding_mode, 6)
    fast = compile_module(net, mode=mode, input_range=1.0)
    calls = []
    inner = fast.ctx.forward_f32_dev
    fast.ctx.forward_f32_dev = lambda *a: (calls.append(a), inner(*a))[1]
    try:
        h, w = 45, 83
        x = batch(channels, 2, w, h)
        ref = module_reference(net, x)
        # a channel-strided view: every second plane of a tensor with twice the channels
        wide = torch.full((2, 2 * channels, h, w), float("nan"))
        wide[:, ::2] = x
        parent = wide.cuda()
        view = parent[:, ::2]
        assert view.stride(1) == 2 * h * w and (channels == 1 or not view.is_contiguous())
        check(fast(view).cpu().numpy(), ref, 1.0, "channel-strided")
        assert calls[-1][0] == view.data_ptr() == parent.data_ptr()
        assert calls[-1][1:4] == (w, 2 * h * w if channels > 1 else 0, 2 * channels * h * w)
        # a row-strided view: a window of a wider and taller tensor (1 channel: the channel pitch is not used)
        big = torch.full((2, channels, h + 7, w + 21), float("nan"))
        big[:, :, 3:3 + h, 10:10 + w] = x
        parent = big.cuda()
        view = parent[:, :, 3:3 + h, 10:10 + w]
        assert not view.is_contiguous() and view.stride(2) == w + 21
        check(fast(view).cpu().numpy(), ref, 1.0, "row-strided")
        assert calls[-1][0] == view.data_ptr() == parent.data_ptr() + 4 * (3 * (w + 21) + 10)
        assert calls[-1][1:4] == (w + 21, (h + 7) * (w + 21) if channels > 1 else 0, channels * (h + 7) * (w + 21))
        n_calls = len(calls)
        with pytest.raises(ValueError):
            fast(x.cuda().permute(0, 1, 3, 2))                # innermost dimension not contiguous
        with pytest.raises(ValueError):
            fast(torch.zeros(2, 4 - channels, h, w).cuda())   # wrong channel count
        with pytest.raises(ValueError):
            fast(x)                                           # a CPU tensor
        assert len(calls) == n_calls, "a refused tensor reaches no call of the library"
    finally:
        fast.close()


def test_module_on_a_non_default_stream_and_two_modules_alive():
    net_a, net_b = make_module(1, 3, "replicate", 7), make_module(3, 1, "zeros", 8)
    fast_a, fast_b = compile_module(net_a), compile_module(net_b, mode=S.MODE_BANDED16)
    try:
        xa, xb = batch(1, 2, 140, 90), batch(3, 2, 64, 50)
        da, db = xa.cuda(), xb.cuda()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ga = fast_a(da)
            gb = fast_b(db)
            ga2 = fast_a(da)
        stream.synchronize()                                  # the results are read only after THAT stream is done
        check(ga.cpu().numpy(), module_reference(net_a, xa), 1.0, "module a")
        check(gb.cpu().numpy(), module_reference(net_b, xb), 1.0, "module b")
        assert torch.equal(ga, ga2)
        # and on the default stream, interleaved with torch's own work on it
        gd = fast_a(da * 0.5) * 2.0
        check(gd.cpu().numpy() / 2.0, module_reference(net_a, xa * 0.5), 1.0, "default stream")
    finally:
        fast_a.close()
        fast_b.close()


# ---- 12: the device form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_device_form_strides_pitches_guards_and_frames(fctx, channels):
    model = make_model(channels, 3, 3)
    fctx.set_model(*model)
    fctx.set_padding("zero")
    fctx.set_input_range(1.0)
    w, h, n = 133, 47, 4
    ss, sc = w + 29, (w + 29) * h + 77                        # source row stride, channel pitch, frame pitch (floats)
    sf = channels * sc + 13
    ds, dc = w + 16, (w + 16) * h + 40
    df = channels * dc + 24
    lead = 32                                                 # guard floats in front of the destination
    xs = [unit_planes(channels, w, h, frame=20 + k) for k in range(n)]
    src = np.full(sf * n, np.float32(7.0))
    for k in range(n):
        for c in range(channels):
            for y in range(h):
                o = k * sf + c * sc + y * ss
                src[o:o + w] = xs[k][c, y]
    GUARD = np.float32(-12345.0)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((lead + df * n + 64,), float(GUARD), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for mode in MODES:
        fctx.set_mode(mode)
        d_dst.fill_(float(GUARD))
        torch.cuda.synchronize()
        fctx.forward_f32_dev(d_src.data_ptr(), ss, sc, sf, d_dst.data_ptr() + 4 * lead, ds, dc, df, w, h, n)
        fctx.synchronize()
        dst = d_dst.cpu().numpy()
        mask = np.ones(dst.size, bool)
        outs = []
        for k in range(n):
            planes = np.empty((channels, h, w), np.float32)
            for c in range(channels):
                for y in range(h):
                    o = lead + k * df + c * dc + y * ds
                    planes[c, y] = dst[o:o + w]
                    mask[o:o + w] = False
            check(planes, reference(xs[k], model, "zero"), 1.0, f"frame {k} mode {mode}")
            outs.append(planes)
        assert (dst[mask] == GUARD).all(), "floats between rows, planes and frames, and around the destination, stay untouched"
        # n_frames = 4 equals four single calls, bit for bit
        for k in range(n):
            d_one = torch.full((channels * dc,), float(GUARD), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            fctx.forward_f32_dev(d_src.data_ptr() + 4 * k * sf, ss, sc, 0, d_one.data_ptr(), ds, dc, 0, w, h, 1)
            fctx.synchronize()
            one = d_one.cpu().numpy()
            for c in range(channels):
                for y in range(h):
                    assert np.array_equal(one[c * dc + y * ds:c * dc + y * ds + w], outs[k][c, y])


# ---- 13: refusals ---------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("channels", [1, 3])
def test_refusals_leave_the_context_usable(fctx, weights_blob, channels):
    model = make_model(channels, 3, 4)
    fctx.set_model(*model)
    w, h = 64, 32
    x = unit_planes(channels, w, h)
    img = synth_color(w, h) if channels == 3 else synth_luma(w, h)
    byte_call = (lambda: fctx.forward_color(img)) if channels == 3 else (lambda: fctx.forward_y(img))
    before = byte_call()
    for mode in OTHER_MODES:
        fctx.set_mode(mode)
        msg = _err(lambda: run(fctx, x), S.ERR_STATE)
        assert f"mode {mode}" in msg and "SRCNN_MODE_MFMA" in msg, msg
        d = torch.from_numpy(x).cuda()
        o = torch.zeros_like(d)
        torch.cuda.synchronize()
        msg = _err(lambda: fctx.forward_f32_dev(d.data_ptr(), w, w * h, 0, o.data_ptr(), w, w * h, 0, w, h, 1), S.ERR_STATE)
        assert f"mode {mode}" in msg, msg
    fctx.set_mode(S.MODE_MFMA)
    # wrong shapes: the binding (ValueError) and the C side (SRCNN_ERR_INVALID) both refuse, with a message
    with pytest.raises(ValueError):
        fctx.forward_f32(np.zeros((4 - channels, h, w), np.float32))
    d = torch.from_numpy(x).cuda()
    o = torch.zeros_like(d)
    torch.cuda.synchronize()
    p, q, pl = d.data_ptr(), o.data_ptr(), w * h
    for bad in (lambda: fctx.forward_f32_dev(0, w, pl, 0, q, w, pl, 0, w, h, 1),             # null source
                lambda: fctx.forward_f32_dev(p, w, pl, 0, 0, w, pl, 0, w, h, 1),             # null destination
                lambda: fctx.forward_f32_dev(p, w, pl, 0, q, w, pl, 0, 0, h, 1),             # width 0
                lambda: fctx.forward_f32_dev(p, w, pl, 0, q, w, pl, 0, w, -1, 1),            # negative height
                lambda: fctx.forward_f32_dev(p, w, pl, 0, q, w, pl, 0, w, h, 0),             # no frames
                lambda: fctx.forward_f32_dev(p, w - 1, pl, 0, q, w, pl, 0, w, h, 1),         # source stride below the width
                lambda: fctx.forward_f32_dev(p, w, pl, 0, q, w - 1, pl, 0, w, h, 1),         # destination stride below the width
                lambda: fctx.forward_f32_dev(p, w, pl, 0, p, w, pl, 0, w, h, 1),             # in place
                lambda: fctx.forward_f32_dev(p, w, pl, 0, q, w, pl, 0, w, h, 2)):            # two frames written to one place
        assert "forward_f32" in _err(bad, S.ERR_INVALID)
    if channels == 3:
        assert "overlap" in _err(lambda: fctx.forward_f32_dev(p, w, pl, 0, q, w, pl // 2, 0, w, h, 1), S.ERR_INVALID)
    assert np.array_equal(byte_call(), before), "the byte call after the refusals gives the bytes it gave before"
    check(run(fctx, x), reference(x, model, "replicate"), 1.0)        # and the float call still runs the model


def test_per_filter_loaded_layers_are_refused(fctx, weights_blob):
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    y = synth_luma(96, 40)
    planes = [np.empty(y.shape, np.float32) for _ in range(32)]
    dst = np.empty_like(y)
    fctx.conv99x11(y, planes, w1, b1, w2, b2)
    fctx.conv55(planes, dst, w3, b3)
    before = fctx.forward_y(y)                                # both layers are loaded: the byte path runs them
    for mode in MODES:
        fctx.set_mode(mode)
        msg = _err(lambda: fctx.forward_f32(y.astype(np.float32)), S.ERR_STATE)
        assert "per-filter" in msg, msg
    fctx.set_mode(S.MODE_MFMA)
    assert np.array_equal(fctx.forward_y(y), before)
    fctx.set_weights_blob(weights_blob)                       # a whole model again: the float call runs
    x = y.astype(np.float32)
    model = S.split_weights(weights_blob)
    check(fctx.forward_f32(x)[None], reference(x[None], model, "replicate"), 255.0)


# ---- 14: the range --------------------------------------------------------------------------------------------------------
def test_input_range_setting(fctx):
    assert fctx.input_range() == 255.0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "srcnn_set_input_range" in _err(lambda: fctx.set_input_range(bad), S.ERR_INVALID)
    assert fctx.input_range() == 255.0
    fctx.set_input_range(1.0)
    fctx.set_model(*random_model(5, 9))                       # the setting survives a model load
    assert fctx.input_range() == 1.0
    fctx.set_model(*random_color_model(1, 9))
    assert fctx.input_range() == 1.0


@pytest.mark.parametrize("channels", [1, 3])
def test_range_one_in_banded16_and_the_byte_path_keeps_its_bytes(fctx, channels):
    model = make_model(channels, 5, 5)
    fctx.set_model(*model)
    fctx.set_padding("zero")
    fctx.set_mode(S.MODE_BANDED16)
    w, h = 300, 170
    img = synth_color(w, h, frame=1) if channels == 3 else synth_luma(w, h, frame=1)
    byte_call = (lambda: fctx.forward_color(img)) if channels == 3 else (lambda: fctx.forward_y(img))
    before = byte_call()
    x = unit_planes(channels, w, h, frame=1)
    ref = reference(x, model, "zero")
    for r in (1.0, 4.0):                                      # a range at and above the data's
        fctx.set_input_range(r)
        check(run(fctx, x), ref, 1.0, f"range {r}")
        assert np.array_equal(byte_call(), before), "the byte entry points keep 255 whatever the range is"
    fctx.set_input_range(255.0)
    assert np.array_equal(byte_call(), before)
