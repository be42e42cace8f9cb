"""9-3-5 / 9-5-5 models on the GPU (srcnn_set_model): the spatial layer-2 MFMA path against a float64 conv2d restatement,
structure tests with a known answer, f2 = 1 through srcnn_set_model, batches and the pipeline, and the refusals."""
from pathlib import Path

import numpy as np
import pytest

import oracle
import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from spatial_reference import (assert_u8_consistent, pre_tolerance, random_model, torch_forward, torch_forward_rows,
                               torch_layer3, torch_layers12)

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
SMALL_SIZES = [(1, 1), (3, 3), (9, 5), (5, 9), (17, 4), (130, 700), (260, 75)]
ALL_MODES = [S.MODE_MFMA, S.MODE_EXACT, S.MODE_SPLIT16, S.MODE_REFBYTES, S.MODE_REFBYTES16]


@pytest.fixture(scope="module")
def sctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _mfma_mode(sctx):
    sctx.set_mode(S.MODE_MFMA)
    yield


def butterfly():
    return np.fromfile(GOLD / "butterfly_y_in_576.u8", np.uint8).reshape(576, 576)


def run(ctx, y):
    pre = np.empty(y.shape, np.float32)
    out = ctx.forward_y(y, preclamp=pre)
    return out, pre


def check(out, pre, ref):
    tol = pre_tolerance(ref)
    assert np.abs(pre.astype(np.float64) - ref).max() <= tol
    assert_u8_consistent(out, ref, tol)


@pytest.mark.parametrize("f2", [3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_matches_float64_small_and_odd_sizes(sctx, f2, seed):
    model = random_model(f2, seed)
    sctx.set_model(*model)
    assert sctx.model_f2() == f2
    for w, h in SMALL_SIZES:
        y = synth_luma(w, h, frame=seed)
        out, pre = run(sctx, y)
        ref = torch_forward(y, model)
        assert np.abs(ref).max() < 2000          # the model does not saturate: the test sees real values
        check(out, pre, ref)


@pytest.mark.parametrize("f2", [3, 5])
def test_matches_float64_1920x1080(sctx, f2):
    model = random_model(f2, 7)
    sctx.set_model(*model)
    y = synth_luma(1920, 1080, frame=3)
    out, pre = run(sctx, y)
    check(out, pre, torch_forward(y, model))


@pytest.mark.parametrize("f2", [3, 5])
def test_matches_float64_3840x2160_row_windows(sctx, f2):
    """Several bands of the plane (the context cuts a 4K plane into row bands): every window's reference comes from only the
    input rows it needs, so only true image edges are replicated."""
    model = random_model(f2, 11)
    sctx.set_model(*model)
    y = synth_luma(3840, 2160, frame=5)
    out, pre = run(sctx, y)
    for r0, r1 in [(0, 40), (300, 340), (1070, 1100), (1500, 1530), (2120, 2160)]:
        ref = torch_forward_rows(y, model, r0, r1)
        check(out[r0:r1], pre[r0:r1], ref)


def test_centre_tap_equals_the_9_1_5_model(sctx):
    model = list(random_model(5, 4))
    w2_1 = random_model(1, 4)[2]
    w2 = np.zeros((32, 64, 5, 5), np.float32)
    w2[:, :, 2, 2] = w2_1
    model[2] = w2
    base = list(model)
    base[2] = w2_1
    y = synth_luma(300, 70, frame=2)
    sctx.set_model(*model)
    out5, pre5 = run(sctx, y)
    sctx.set_weights(*base)
    assert sctx.model_f2() == 1
    out1, pre1 = run(sctx, y)
    ref = torch_forward(y, base)
    tol = pre_tolerance(ref)
    assert np.abs(pre5.astype(np.float64) - pre1).max() <= tol
    check(out5, pre5, ref)


@pytest.mark.parametrize("kh,kw", [(0, 3), (4, 0), (1, 4)])
def test_off_centre_tap_shifts_the_map_with_replicate_edges(sctx, kh, kw):
    """One-hot tap (kh, kw): the layer-2 map is the 9-1-5 map shifted by (kh - 2, kw - 2), edges replicated; a flipped or
    transposed kernel or a wrong border fails here."""
    model = list(random_model(5, 5))
    w2_1 = random_model(1, 5)[2]
    w2 = np.zeros((32, 64, 5, 5), np.float32)
    w2[:, :, kh, kw] = w2_1
    model[2] = w2
    base = list(model)
    base[2] = w2_1
    h, w = 70, 131
    y = synth_luma(w, h, frame=6)
    m1 = torch_layers12(y, base).numpy()
    ys = np.clip(np.arange(h) + kh - 2, 0, h - 1)[:, None]
    xs = np.clip(np.arange(w) + kw - 2, 0, w - 1)[None, :]
    ref = torch_layer3(m1[:, ys, xs], model)
    sctx.set_model(*model)
    out, pre = run(sctx, y)
    check(out, pre, ref)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_f2_1_through_set_model_is_set_weights(sctx, weights_blob, mode):
    y = butterfly()
    w = S.split_weights(weights_blob)
    sctx.set_weights(*w)
    sctx.set_mode(mode)
    a = sctx.forward_y(y)
    sctx.set_model(*w)
    assert sctx.model_f2() == 1
    b = sctx.forward_y(y)
    assert np.array_equal(a, b)
    if mode in (S.MODE_MFMA, S.MODE_EXACT):
        pa, pb = np.empty(y.shape, np.float32), np.empty(y.shape, np.float32)
        sctx.set_weights(*w)
        sctx.forward_y(y, preclamp=pa)
        sctx.set_model(*w)
        sctx.forward_y(y, preclamp=pb)
        assert np.array_equal(pa, pb)


def _torch():
    import torch
    return torch


def test_device_batch_with_frame_pitches_equals_single_calls(sctx):
    torch = _torch()
    model = random_model(5, 8)
    sctx.set_model(*model)
    w, h, n = 203, 97, 3
    sstride, dstride = 256, 224
    spitch, dpitch = sstride * h + 96, dstride * h + 32
    frames = np.stack([synth_luma(w, h, frame=k) for k in range(n)])
    src = torch.zeros(n * spitch, dtype=torch.uint8)
    for k in range(n):
        src[k * spitch:k * spitch + sstride * h].view(h, sstride)[:, :w] = torch.from_numpy(frames[k])
    d_src = src.cuda()
    d_dst = torch.zeros(n * dpitch, dtype=torch.uint8, device="cuda")
    d_one = torch.zeros(n * dpitch, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sctx.forward_y_dev(d_src.data_ptr(), sstride, spitch, d_dst.data_ptr(), dstride, dpitch, w, h, n)
    for k in range(n):
        sctx.forward_y_dev(d_src.data_ptr() + k * spitch, sstride, 0, d_one.data_ptr() + k * dpitch, dstride, 0, w, h, 1)
    sctx.synchronize()
    batch, single = d_dst.cpu().numpy(), d_one.cpu().numpy()
    assert np.array_equal(batch, single)
    outs = [single[k * dpitch:k * dpitch + dstride * h].reshape(h, dstride)[:, :w] for k in range(n)]
    assert np.array_equal(np.stack(outs), sctx.forward_y_frames(frames))
    for k in range(n):
        assert np.array_equal(outs[k], sctx.forward_y(frames[k]))
    check(outs[1], run(sctx, frames[1])[1], torch_forward(frames[1], model))


def test_device_preclamp(sctx):
    torch = _torch()
    model = random_model(3, 9)
    sctx.set_model(*model)
    y = synth_luma(150, 40, frame=1)
    d_src = torch.from_numpy(y).cuda()
    d_dst = torch.zeros_like(d_src)
    d_pre = torch.zeros(y.shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sctx.forward_y_dev(d_src.data_ptr(), 150, 0, d_dst.data_ptr(), 150, 0, 150, 40, 1, d_pre.data_ptr())
    sctx.synchronize()
    out, pre = run(sctx, y)
    assert np.array_equal(d_dst.cpu().numpy(), out) and np.array_equal(d_pre.cpu().numpy(), pre)


def test_process_bgr_equals_the_composed_steps(sctx):
    model = random_model(5, 10)
    sctx.set_model(*model)
    rng = np.random.default_rng(3)
    bgr = (rng.integers(0, 256, (61, 83, 3)) // 8 * 8).astype(np.uint8)
    scale = 1.5
    ow, oh = S.scaled_size(83, 61, scale)
    planes = [sctx.resize_cubic(p, ow, oh) for p in sctx.bgr2ycrcb(bgr)]
    want = sctx.ycrcb2bgr(sctx.forward_y(planes[0]), planes[1], planes[2])
    assert np.array_equal(sctx.process_bgr(bgr, scale), want)
    torch = _torch()
    d_in = torch.from_numpy(bgr).cuda()
    d_out = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sctx.process_bgr_dev(d_in.data_ptr(), 3 * 83, 83, 61, scale, d_out.data_ptr(), 3 * ow)
    sctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)


def _state(fn):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == S.ERR_STATE
    return str(e.value)


def test_refusals(sctx):
    torch = _torch()
    sctx.set_model(*random_model(5, 12))
    w, h = 64, 32
    y = synth_luma(w, h)
    d_src = torch.from_numpy(y).cuda()
    d_dst = torch.zeros_like(d_src)
    d_work = torch.zeros(32 * w * h, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p, o = d_src.data_ptr(), d_dst.data_ptr()
    _state(lambda: sctx.forward_y_rows_dev(p, w, 0, o, w, 0, w, h, 0, h))
    _state(lambda: sctx.forward_y_rows_halo_dev(p, w, 0, h, 0, 0, w, o, w, 0, w, h, 0, h))
    _state(lambda: sctx.forward_y_unfused_dev(p, w, 0, o, w, 0, w, h, 1, d_work.data_ptr()))
    _state(lambda: sctx.conv99x11_dev(p, w, d_work.data_ptr(), w, w * h, w, h))
    _state(lambda: sctx.conv55_dev(d_work.data_ptr(), w, w * h, o, w, w, h))
    _state(lambda: S.forward_y_striped([sctx], y))
    _state(lambda: S.forward_y_striped_frames([sctx], y[None]))
    _state(lambda: S.forward_y_frames_multi([sctx], y[None]))
    _state(lambda: S.forward_y_lanes_dev([sctx], [p], w, [o], w, w, h))
    _state(lambda: S.forward_y_striped_dev([sctx], [p], w, [o], w, w, h))
    assert sctx.model_f2() == 5
    for mode in ALL_MODES[1:]:
        sctx.set_mode(mode)
        msg = _state(lambda: sctx.forward_y(y))
        assert "SRCNN_MODE_MFMA" in msg
        _state(lambda: sctx.forward_y_frames(y[None]))
    sctx.set_mode(S.MODE_MFMA)
    assert sctx.model_f2() == 5
    sctx.forward_y(y)                            # the model is still there and runs


def test_per_filter_calls(sctx, weights_blob):
    """Documented rule (srcnn_set_model): srcnn_conv99 / srcnn_conv11 leave the model intact; a per-filter call that loads
    weights (srcnn_conv55, srcnn_conv99x11) ends it, and the whole path then refuses until a model is loaded again."""
    model = random_model(5, 13)
    sctx.set_model(*model)
    y = synth_luma(70, 30, frame=4)
    before = sctx.forward_y(y)
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    sctx.conv99(y, np.empty(y.shape, np.float32), w1[0], float(b1[0]))
    sctx.conv11([np.ones(y.shape, np.float32)] * 64, np.empty(y.shape, np.float32), w2[0], float(b2[0]))
    assert sctx.model_f2() == 5
    assert np.array_equal(sctx.forward_y(y), before)
    sctx.conv55([np.ones(y.shape, np.float32)] * 32, np.empty(y.shape, np.uint8), w3, b3)
    assert sctx.model_f2() == 1
    _state(lambda: sctx.forward_y(y))
    sctx.set_model(*model)
    assert np.array_equal(sctx.forward_y(y), before)
    sctx.conv99x11(y, [np.empty(y.shape, np.float32) for _ in range(32)], w1, b1, w2, b2)
    assert sctx.model_f2() == 1
    _state(lambda: sctx.forward_y(y))


def test_no_state_leaks_back_to_the_9_1_5_model(sctx, weights_blob):
    sctx.set_model(*random_model(5, 14))
    sctx.forward_y(synth_luma(100, 50))
    sctx.set_weights_blob(weights_blob)
    assert sctx.model_f2() == 1
    sctx.set_mode(S.MODE_REFBYTES)
    y = butterfly()
    r_out, _ = oracle.forward_y(y, weights_blob)
    assert np.array_equal(sctx.forward_y(y), r_out)
