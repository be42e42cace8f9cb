"""Layer 2 of a wide model in split f16 on the GPU (srcnn_set_wide_split16; spatial_l2h_kernel's wide forms): float64 references at the
tile edges of all three layers, two bitwise links to what already runs (a 64 / 32 model zero-embedded in wider tensors gives
SRCNN_MODE_BANDED16's bytes and floats; one-hot hidden channels), the band seam of a 1024 x 768 plane, the float path's input
range and compile_module(mode=MODE_BANDED16) on a 128 / 64 module, and that nothing else moves: narrow models, the refusals, the
option switched off again, a model the split cannot scale.

Tolerance against float64, as tests/test_gpu_wide.py: pre_tolerance(ref) * max(n1p / 64, n2p / 32)."""
import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from srcnn_cpp_amd.torch_api import compile_module
from spatial_reference import assert_u8_consistent
from test_gpu_wide import (PADDINGS, SIZES, byte_planes, check_against_float64, float_planes, module64, one_hot_model, run_f32, run_u8,
                           tolerance, unit_tolerance, wide_module)
from wide_reference import as_plain, band_seams, embed, forward, forward_rows, random_wide_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(hctx):
    def reset():
        hctx.set_mode(S.MODE_MFMA)
        hctx.set_padding("replicate")
        hctx.set_input_range(255.0)
        hctx.set_wide_split16(False)
    reset()
    yield
    reset()


def test_the_option_is_a_setting_of_the_context(hctx):
    assert hctx.wide_split16() is False
    hctx.set_wide_split16(True)
    assert hctx.wide_split16() is True
    for model in (random_wide_model(1, 128, 3, 64, 1), as_plain(random_wide_model(1, 64, 3, 32, 1)), random_wide_model(3, 64, 1, 64, 1)):
        hctx.set_model(*model)
        assert hctx.wide_split16() is True                     # it survives every loader, like the padding
    assert hctx._lib.srcnn_set_wide_split16(hctx._h, 2) == S.ERR_INVALID and hctx._lib.srcnn_set_wide_split16(hctx._h, -1) == S.ERR_INVALID
    assert "srcnn_set_wide_split16" in hctx._lib.srcnn_last_error(hctx._h).decode()
    assert hctx.wide_split16() is True
    hctx.set_wide_split16(False)
    assert hctx.wide_split16() is False


# ---- 1: against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_128_64_matches_float64(hctx, channels, f2, padding):
    model = random_wide_model(channels, 128, f2, 64, 1)
    hctx.set_model(*model)
    hctx.set_padding(padding)
    hctx.set_wide_split16(True)
    check_against_float64(hctx, model, channels, 128, 64, padding, SIZES, f"split16 128/64 {channels}ch 9-{f2}-5 {padding}")


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n1,n2", [(128, 32), (64, 64), (96, 48), (100, 40)])
def test_other_widths_match_float64(hctx, n1, n2, channels, padding):
    model = random_wide_model(channels, n1, 3, n2, 2)
    hctx.set_model(*model)
    hctx.set_padding(padding)
    hctx.set_wide_split16(True)
    check_against_float64(hctx, model, channels, n1, n2, padding, [(130, 67)], f"split16 {n1}/{n2} {channels}ch 9-3-5 {padding}")


def test_the_split_form_is_not_the_f32_form(hctx):
    """The option does switch kernels: the two forms agree within the tolerance and differ in the last bits."""
    model = random_wide_model(1, 128, 3, 64, 1)
    hctx.set_model(*model)
    x = float_planes(1, 130, 67, frame=1)
    f32 = run_f32(hctx, x)
    hctx.set_wide_split16(True)
    f16 = run_f32(hctx, x)
    ref = forward(x, model)
    assert not np.array_equal(f16, f32)
    assert np.abs(f16.astype(np.float64) - ref).max() <= tolerance(ref, 128, 64)


# ---- 2: a 64 / 32 model embedded in wider tensors gives the bytes and floats of SRCNN_MODE_BANDED16 -----------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_zero_embedded_64_32_model_is_bitwise_banded16(hctx, channels, f2, padding):
    """The real channels first, zeros after: the extra K steps and output groups add exact zeros, and the two scales do not move
    (a zero channel has a zero bound, a zero weight does not raise max |W2|).  So the kernel's summation order is
    spatial_l2h_kernel's continued if and only if everything is equal (+0 equals -0)."""
    w, h = 130, 67
    model = random_wide_model(channels, 64, f2, 32, 3)
    xb, xf = byte_planes(channels, w, h, frame=f2), float_planes(channels, w, h, frame=f2)
    hctx.set_padding(padding)
    hctx.set_model(*as_plain(model))
    hctx.set_mode(S.MODE_BANDED16)
    want_out, want_pre = run_u8(hctx, xb)
    want_f = run_f32(hctx, xf)
    assert len(np.unique(want_f)) > h
    hctx.set_mode(S.MODE_MFMA)
    hctx.set_wide_split16(True)
    for n1, n2 in [(128, 64), (128, 32), (64, 64)]:
        hctx.set_model(*embed(model, n1, n2))
        assert hctx.model_shape() == (channels, n1, f2, n2)
        out, pre = run_u8(hctx, xb)
        assert np.array_equal(out, want_out), (n1, n2)
        assert np.array_equal(pre, want_pre), (n1, n2, np.abs(pre - want_pre).max())
        got = run_f32(hctx, xf)
        assert np.array_equal(got, want_f), (n1, n2, np.abs(got - want_f).max())


# ---- 3: one-hot hidden channels: any step, group or table offset error shows exactly --------------------------------------
@pytest.mark.parametrize("k1,k2", [(127, 63), (64, 32), (65, 33), (63, 31)])
@pytest.mark.parametrize("channels,f2,padding", [(1, 1, "replicate"), (1, 3, "zero"), (1, 5, "replicate"), (3, 1, "zero"),
                                                 (3, 3, "replicate"), (3, 5, "zero")])
def test_one_hot_channels_equal_the_pair_moved_to_0_0(hctx, channels, f2, padding, k1, k2):
    """One live channel per layer with the same values wherever it sits: the same scales, one non-zero product per MFMA (the
    others are exact zeros, so the order inside the instruction does not matter), the same three products per tap."""
    x = float_planes(channels, 130, 67, frame=1)
    hctx.set_padding(padding)
    hctx.set_wide_split16(True)
    hctx.set_model(*one_hot_model(channels, f2, 0, 0))
    want = run_f32(hctx, x)
    assert len(np.unique(want)) > 67, "the hidden channels are alive"
    hctx.set_model(*one_hot_model(channels, f2, k1, k2))
    got = run_f32(hctx, x)
    assert np.array_equal(got, want), np.abs(got - want).max()
    ref = forward(x, one_hot_model(channels, f2, k1, k2), padding)
    assert np.abs(got - ref).max() <= tolerance(ref, 128, 64)


# ---- 4: the band seam -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f2,channels,padding", [(3, 1, "replicate"), (5, 3, "zero")])
def test_1024x768_rows_across_the_band_seam(hctx, f2, channels, padding):
    """Two bands with the seam at row 384: rows 372 .. 396 against the float64 reference of that row window with its halo, so
    that only true image edges are padded."""
    w, h = 1024, 768
    model = random_wide_model(channels, 128, f2, 64, 6)
    hctx.set_model(*model)
    hctx.set_padding(padding)
    hctx.set_wide_split16(True)
    assert band_seams(w, h, f2, 128, 64) == [384]
    xb, xf = byte_planes(channels, w, h, frame=4), float_planes(channels, w, h, frame=5)
    out, pre = run_u8(hctx, xb)
    got = run_f32(hctx, xf)
    r0, r1 = 372, 397
    ref = forward_rows(xb, model, r0, r1, padding)
    tol = tolerance(ref, 128, 64)
    err = np.abs(pre[:, r0:r1].astype(np.float64) - ref).max()
    assert err <= tol, f"bytes, rows {r0}..{r1 - 1}: error {err:.3g}, tolerance {tol:.3g}"
    assert_u8_consistent(out[:, r0:r1], ref, tol)
    ref = forward_rows(xf, model, r0, r1, padding)
    errf = np.abs(got[:, r0:r1].astype(np.float64) - ref).max()
    assert errf <= tolerance(ref, 128, 64), f"floats, rows {r0}..{r1 - 1}: error {errf:.3g}"
    print(f"seam 9-{f2}-5 {channels}ch {padding}: largest error {max(err, errf):.3g} (tolerance {tol:.3g})")


# ---- 5: the float path's input range --------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,f2,padding", [(1, 3, "replicate"), (3, 5, "zero")])
def test_unit_range_planes_with_input_range_1(hctx, channels, f2, padding):
    """Planes in 0 .. 1 through a model for such data (layer 1 times 255, layer 3 over 255), srcnn_set_input_range(1.0): the
    layer-1 scale follows the range, and the error is that of 0 .. 255 data carried over by homogeneity."""
    w1, b1, w2, b2, w3, b3 = random_wide_model(channels, 128, f2, 64, 7)
    model = ((w1 * np.float32(255.0)).astype(np.float32), b1, w2, b2, (w3 / np.float32(255.0)).astype(np.float32),
             (b3 / np.float32(255.0)).astype(np.float32))
    x = (float_planes(channels, 130, 67, frame=2) / np.float32(255.0)).astype(np.float32)
    assert x.max() <= 1.0
    hctx.set_model(*model)
    hctx.set_padding(padding)
    hctx.set_input_range(1.0)
    hctx.set_wide_split16(True)
    got = run_f32(hctx, x)
    ref = forward(x, model, padding)
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"unit range {channels}ch 9-{f2}-5 {padding}: error {err:.3g}, tolerance {unit_tolerance(ref):.3g}")
    assert np.isfinite(got).all() and err <= unit_tolerance(ref)


@pytest.mark.parametrize("channels,f2,padding_mode", [(1, 3, "zeros"), (3, 5, "replicate")])
def test_compile_module_banded16_on_a_wide_module(channels, f2, padding_mode):
    """mode=MODE_BANDED16 is the fast mode for every width: a 128 / 64 module keeps its context in MODE_MFMA with the option on."""
    net = wide_module(channels, f2, padding_mode, 5)
    fast = compile_module(net, device=0, mode=S.MODE_BANDED16, input_range=1.0)
    slow = compile_module(net, device=0, mode=S.MODE_MFMA)
    try:
        assert fast.ctx.model_shape() == (channels, 128, f2, 64)
        assert fast.ctx._lib.srcnn_get_mode(fast.ctx._h) == S.MODE_MFMA and fast.ctx.wide_split16() is True
        assert fast.ctx.input_range() == 1.0
        assert slow.ctx._lib.srcnn_get_mode(slow.ctx._h) == S.MODE_MFMA and slow.ctx.wide_split16() is False     # unchanged
        x = torch.from_numpy(np.stack([float_planes(channels, 97, 61, frame=k) / np.float32(255.0) for k in range(2)]))
        got = fast(x.cuda())
        assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda
        ref = module64(net, x)
        err = np.abs(got.cpu().numpy() - ref).max()
        assert err <= unit_tolerance(ref), f"error {err:.3g}, tolerance {unit_tolerance(ref):.3g}"
        assert not torch.equal(got, slow(x.cuda()))             # the split form did run
    finally:
        fast.close()
        slow.close()


def test_compile_module_banded16_on_a_narrow_module_keeps_the_mode():
    torch.manual_seed(3)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(1, 64, 9, padding=4)
            self.conv2 = torch.nn.Conv2d(64, 32, 3, padding=1)
            self.conv3 = torch.nn.Conv2d(32, 1, 5, padding=2)

    fast = compile_module(Net().eval(), device=0, mode=S.MODE_BANDED16, input_range=1.0)
    try:
        assert fast.ctx._lib.srcnn_get_mode(fast.ctx._h) == S.MODE_BANDED16 and fast.ctx.wide_split16() is False
    finally:
        fast.close()


# ---- 6: nothing else moves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [S.MODE_MFMA, S.MODE_BANDED16])
@pytest.mark.parametrize("channels,f2", [(1, 1), (1, 3), (3, 5)])
def test_a_narrow_model_ignores_the_option(hctx, mode, channels, f2):
    x = byte_planes(channels, 130, 67, frame=1)
    hctx.set_model(*random_wide_model(channels, 32, f2, 16, 12))
    hctx.set_mode(mode)
    want = run_u8(hctx, x)
    want_f = run_f32(hctx, x.astype(np.float32))
    hctx.set_wide_split16(True)
    got = run_u8(hctx, x)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(run_f32(hctx, x.astype(np.float32)).view(np.uint32), want_f.view(np.uint32))


def _state(fn):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == S.ERR_STATE
    return str(e.value)


def test_refusals_stay_and_switching_off_returns_the_f32_bytes(hctx):
    model = random_wide_model(1, 128, 3, 64, 13)
    hctx.set_model(*model)
    w, h = 64, 32
    y = synth_luma(w, h)
    before = hctx.forward_y(y)
    hctx.set_wide_split16(True)
    split = hctx.forward_y(y)
    d_src = torch.from_numpy(y).cuda()
    d_dst = torch.zeros_like(d_src)
    torch.cuda.synchronize()
    p, o = d_src.data_ptr(), d_dst.data_ptr()
    msg = _state(lambda: hctx.model_rows_dev(p, w, 0, o, w, 0, w, h, 0, h))
    assert "128" in msg and "64" in msg, msg
    for mode in (S.MODE_BANDED16, S.MODE_SPLIT16):
        hctx.set_mode(mode)
        for call in (lambda: hctx.forward_y(y), lambda: hctx.forward_f32(y.astype(np.float32))):
            msg = _state(call)
            assert "128" in msg and "64" in msg and "SRCNN_MODE_MFMA" in msg, (mode, msg)
    hctx.set_mode(S.MODE_MFMA)
    assert np.array_equal(hctx.forward_y(y), split)              # the context is still usable, the option still on
    ref = forward(y[None], model)
    assert_u8_consistent(split[None], ref, tolerance(ref, 128, 64))
    hctx.set_wide_split16(False)
    assert np.array_equal(hctx.forward_y(y), before)             # the float32 kernels again


def test_a_model_the_split_cannot_scale_is_refused_and_runs_with_the_option_off(hctx):
    w1, b1, w2, b2, w3, b3 = random_wide_model(1, 128, 3, 64, 14)
    bad = w2.copy()
    bad[63, 127, 1, 1] = np.inf
    y = synth_luma(70, 30, frame=4)
    hctx.set_model(w1, b1, bad, b2, w3, b3)
    hctx.set_wide_split16(True)
    for _ in range(2):                                           # refused at every call, not only the first
        for call in (lambda: hctx.forward_y(y), lambda: hctx.forward_f32(y.astype(np.float32))):
            msg = _state(call)
            assert "srcnn_set_wide_split16" in msg, msg
    hctx.set_wide_split16(False)
    hctx.forward_y(y)                                            # float32 runs it (whatever an infinite weight gives)
    hctx.set_wide_split16(True)
    good = (w1, b1, w2, b2, w3, b3)
    hctx.set_model(*good)                                        # a model that can be scaled replaces it
    ref = forward(y[None], good)
    assert_u8_consistent(hctx.forward_y(y)[None], ref, tolerance(ref, 128, 64))
