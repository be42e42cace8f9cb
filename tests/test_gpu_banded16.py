"""SRCNN_MODE_BANDED16 on the GPU: every whole model on the banded path with layer 2 in split f16 (spatial_l2h_kernel), held to the
tolerance of SRCNN_MODE_MFMA against the float64 restatements; an error at the float32 level; exact structure (batches, frames,
the pipeline, one-hot taps, mode switches); and the refusals.

The tight numerical bound of the mode (and of SRCNN_MODE_MFMA's banded kernels) is in tests/test_gpu_banded_error_level.py: every
kernel form at the tile bounds of the three kernels, within 4 x the error of a plain float32 evaluation (tests/error_level.py)."""
import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from color_reference import random_color_model, synth_color, torch_forward_color, torch_forward_color_rows
from spatial_reference import (assert_u8_consistent, band_seams, pre_tolerance, random_model, torch_forward, torch_forward_rows,
                               torch_layer3, torch_layers12)
from zero_pad_reference import torch_forward_zero, torch_forward_zero_rows

pytestmark = pytest.mark.gpu

SMALL_SIZES = [(1, 1), (3, 3), (9, 5), (5, 9), (17, 4), (130, 700), (260, 75)]
PADDINGS = ["replicate", "zero"]


@pytest.fixture(scope="module")
def bctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _banded16(bctx):
    bctx.set_padding("replicate")
    bctx.set_mode(S.MODE_BANDED16)
    yield
    bctx.set_mode(S.MODE_MFMA)
    bctx.set_padding("replicate")


def run(ctx, y):
    pre = np.empty(y.shape, np.float32)
    out = ctx.forward_y(y, preclamp=pre)
    return out, pre


def run_color(ctx, img):
    pre = np.empty(img.shape, np.float32)
    out = ctx.forward_color(img, preclamp=pre)
    return out, pre


def check(out, pre, ref):
    tol = pre_tolerance(ref)
    err = np.abs(pre.astype(np.float64) - ref).max()
    print(f"max |pre - ref| = {err:.3g} (tolerance {tol:.3g}, max |ref| {np.abs(ref).max():.4g})")
    assert err <= tol
    assert_u8_consistent(out, ref, tol)


def luma_ref(y, model, padding):
    return torch_forward(y, model) if padding == "replicate" else torch_forward_zero(y, model)


# ---- accuracy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_matches_float64_small_and_odd_sizes(bctx, f2, seed, padding):
    model = random_model(f2, seed)
    bctx.set_padding(padding)
    bctx.set_model(*model)
    assert bctx.model_f2() == f2
    for w, h in SMALL_SIZES:
        y = synth_luma(w, h, frame=seed)
        ref = luma_ref(y, model, padding)
        assert np.abs(ref).max() < 2000          # the model does not saturate: the test sees real values
        check(*run(bctx, y), ref)


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [3, 5])
def test_matches_float64_1920x1080(bctx, f2, padding):
    model = random_model(f2, 7)
    bctx.set_padding(padding)
    bctx.set_model(*model)
    y = synth_luma(1920, 1080, frame=3)
    check(*run(bctx, y), luma_ref(y, model, padding))


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_luma_9_1_5_runs_banded(bctx, weights_blob, seed, padding):
    """One rule: every whole model runs banded in this mode, also the 9-1-5 one under replicate padding."""
    model = random_model(1, seed)
    bctx.set_padding(padding)
    bctx.set_model(*model)
    for w, h in SMALL_SIZES + [(640, 360)]:
        y = synth_luma(w, h, frame=seed)
        check(*run(bctx, y), luma_ref(y, model, padding))


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_colour_models_match_float64(bctx, f2, padding):
    model = random_color_model(f2, 1)
    bctx.set_padding(padding)
    bctx.set_model(*model)
    assert bctx.model_channels() == 3 and bctx.model_f2() == f2
    for w, h in SMALL_SIZES + [(640, 360)]:
        img = synth_color(w, h, frame=f2)
        check(*run_color(bctx, img), torch_forward_color(img, model, padding))


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [3, 5])
def test_matches_float64_3840x2160_row_windows(bctx, f2, padding):
    """Several bands of the plane: windows at the image edges, inside the plane and across every band seam, each against a
    reference computed from only the input rows it needs."""
    model = random_model(f2, 11)
    bctx.set_padding(padding)
    bctx.set_model(*model)
    w, h = 3840, 2160
    y = synth_luma(w, h, frame=5)
    out, pre = run(bctx, y)
    seams = band_seams(w, h, f2)
    assert seams
    rows = torch_forward_rows if padding == "replicate" else torch_forward_zero_rows
    for r0, r1 in [(0, 40), (300, 340), (1500, 1530), (h - 40, h)] + [(s - 8, s + 8) for s in seams]:
        check(out[r0:r1], pre[r0:r1], rows(y, model, r0, r1))


def test_colour_3840x2160_row_windows(bctx):
    model = random_color_model(5, 2)
    bctx.set_model(*model)
    w, h = 3840, 2160
    img = synth_color(w, h, frame=3)
    out, pre = run_color(bctx, img)
    seams = band_seams(w, h, 5)
    assert seams
    for r0, r1 in [(0, 12), (h - 12, h)] + [(s - 8, s + 8) for s in seams]:
        check(out[r0:r1], pre[r0:r1], torch_forward_color_rows(img, model, r0, r1, "replicate"))


@pytest.mark.parametrize("f2", [3, 5])
def test_error_is_at_the_float32_level(bctx, f2):
    """The split keeps 22 bits per operand: max and mean error against float64 within a factor 2 of SRCNN_MODE_MFMA's (plus the
    absolute terms of test_split16_is_at_least_as_close_to_the_reference_as_mfma)."""
    model = random_model(f2, 4)
    bctx.set_model(*model)
    w, h = 640, 360
    y = synth_luma(w, h, frame=4)
    ref = torch_forward(y, model)
    _, pre_s = run(bctx, y)
    bctx.set_mode(S.MODE_MFMA)
    _, pre_m = run(bctx, y)
    e_m, e_s = np.abs(pre_m - ref), np.abs(pre_s - ref)
    print(f"9-{f2}-5: BANDED16 max {e_s.max():.3g} mean {e_s.mean():.3g}; MFMA max {e_m.max():.3g} mean {e_m.mean():.3g}")
    assert e_s.max() <= 2 * e_m.max() + 1e-4
    assert e_s.mean() <= 2 * e_m.mean() + 1e-5


# ---- exact structure ----------------------------------------------------------------------------------------------------------
def test_deterministic(bctx):
    bctx.set_model(*random_model(5, 6))
    y = synth_luma(517, 203, frame=2)
    a, pa = run(bctx, y)
    b, pb = run(bctx, y)
    assert np.array_equal(a, b) and np.array_equal(pa, pb)


def test_device_batch_with_frame_pitches_equals_single_calls(bctx):
    model = random_model(5, 8)
    bctx.set_model(*model)
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
    bctx.forward_y_dev(d_src.data_ptr(), sstride, spitch, d_dst.data_ptr(), dstride, dpitch, w, h, n)
    for k in range(n):
        bctx.forward_y_dev(d_src.data_ptr() + k * spitch, sstride, 0, d_one.data_ptr() + k * dpitch, dstride, 0, w, h, 1)
    bctx.synchronize()
    batch, single = d_dst.cpu().numpy(), d_one.cpu().numpy()
    assert np.array_equal(batch, single)
    outs = [single[k * dpitch:k * dpitch + dstride * h].reshape(h, dstride)[:, :w] for k in range(n)]
    assert np.array_equal(np.stack(outs), bctx.forward_y_frames(frames))
    for k in range(n):
        assert np.array_equal(outs[k], bctx.forward_y(frames[k]))
    check(outs[1], run(bctx, frames[1])[1], torch_forward(frames[1], model))


def test_process_bgr_equals_the_composed_steps(bctx):
    bctx.set_model(*random_model(5, 10))
    rng = np.random.default_rng(3)
    bgr = (rng.integers(0, 256, (61, 83, 3)) // 8 * 8).astype(np.uint8)
    scale = 1.5
    ow, oh = S.scaled_size(83, 61, scale)
    planes = [bctx.resize_cubic(p, ow, oh) for p in bctx.bgr2ycrcb(bgr)]
    want = bctx.ycrcb2bgr(bctx.forward_y(planes[0]), planes[1], planes[2])
    assert np.array_equal(bctx.process_bgr(bgr, scale), want)
    d_in = torch.from_numpy(bgr).cuda()
    d_out = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bctx.process_bgr_dev(d_in.data_ptr(), 3 * 83, 83, 61, scale, d_out.data_ptr(), 3 * ow)
    bctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)


def test_process_bgr_with_a_colour_model(bctx):
    model = random_color_model(3, 4)
    bctx.set_model(*model)
    rng = np.random.default_rng(5)
    bgr = (rng.integers(0, 256, (45, 71, 3)) // 8 * 8).astype(np.uint8)
    scale = 2.0
    ow, oh = S.scaled_size(71, 45, scale)
    up = np.ascontiguousarray(np.stack([bctx.resize_cubic(np.ascontiguousarray(bgr[:, :, k]), ow, oh) for k in range(3)], axis=2))
    assert np.array_equal(bctx.process_bgr(bgr, scale), bctx.forward_color(up))


@pytest.mark.parametrize("kh,kw", [(0, 3), (4, 0), (1, 4)])
def test_off_centre_tap_shifts_the_map_with_replicate_edges(bctx, kh, kw):
    """One-hot tap (kh, kw): the layer-2 map is the 9-1-5 map shifted by (kh - 2, kw - 2), edges replicated; a flipped or
    transposed W2 table or a wrong border fails here."""
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
    bctx.set_model(*model)
    check(*run(bctx, y), ref)


def test_one_hot_channel_routing(bctx):
    """W2 = a permutation of 32 of the 64 layer-1 channels on the centre tap: a K slot of the table that holds another channel
    than the map's plane fails here by far more than the tolerance."""
    model = list(random_model(3, 14))
    rng = np.random.default_rng(14)
    pick = rng.permutation(64)[:32]
    w2 = np.zeros((32, 64, 3, 3), np.float32)
    w2[np.arange(32), pick, 1, 1] = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    model[2] = w2
    bctx.set_model(*model)
    y = synth_luma(131, 70, frame=7)
    check(*run(bctx, y), torch_forward(y, model))


@pytest.mark.parametrize("padding", PADDINGS)
def test_mode_switches_leave_no_stale_map_or_table(bctx, padding):
    bctx.set_padding(padding)
    bctx.set_model(*random_model(5, 15))
    y = synth_luma(300, 200, frame=8)
    bctx.set_mode(S.MODE_MFMA)
    first, first_pre = run(bctx, y)
    bctx.set_mode(S.MODE_BANDED16)
    mid, mid_pre = run(bctx, y)
    bctx.set_mode(S.MODE_MFMA)
    again, again_pre = run(bctx, y)
    assert np.array_equal(first, again) and np.array_equal(first_pre, again_pre)
    bctx.set_mode(S.MODE_BANDED16)
    mid2, mid2_pre = run(bctx, y)
    assert np.array_equal(mid, mid2) and np.array_equal(mid_pre, mid2_pre)
    # a new model in the mode: the split table follows it
    model = random_model(3, 16)
    bctx.set_model(*model)
    check(*run(bctx, y), luma_ref(y, model, padding))


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _state(fn):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == S.ERR_STATE
    return str(e.value)


@pytest.mark.parametrize("f2", [1, 5])
def test_refusals(bctx, f2):
    model = random_model(f2, 12)
    bctx.set_model(*model)
    w, h = 64, 32
    y = synth_luma(w, h)
    d_src = torch.from_numpy(y).cuda()
    d_dst = torch.zeros_like(d_src)
    d_work = torch.zeros(32 * w * h, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p, o = d_src.data_ptr(), d_dst.data_ptr()
    msgs = [
        _state(lambda: bctx.forward_y_rows_dev(p, w, 0, o, w, 0, w, h, 0, h)),
        _state(lambda: bctx.forward_y_rows_halo_dev(p, w, 0, h, 0, 0, w, o, w, 0, w, h, 0, h)),
        _state(lambda: bctx.forward_y_unfused_dev(p, w, 0, o, w, 0, w, h, 1, d_work.data_ptr())),
        _state(lambda: bctx.conv99x11_dev(p, w, d_work.data_ptr(), w, w * h, w, h)),
        _state(lambda: bctx.conv55_dev(d_work.data_ptr(), w, w * h, o, w, w, h)),
        _state(lambda: S.forward_y_striped([bctx], y)),
        _state(lambda: S.forward_y_striped_frames([bctx], y[None])),
        _state(lambda: S.forward_y_frames_multi([bctx], y[None])),
        _state(lambda: S.forward_y_lanes_dev([bctx], [p], w, [o], w, w, h)),
        _state(lambda: S.forward_y_striped_dev([bctx], [p], w, [o], w, w, h)),
    ]
    assert all("SRCNN_MODE_BANDED16" in m for m in msgs), msgs
    assert bctx.model_f2() == f2
    check(*run(bctx, y), torch_forward(y, model))           # the model is still there and runs


def test_colour_model_and_luma_entry_points(bctx):
    bctx.set_model(*random_color_model(3, 3))
    y = synth_luma(40, 30)
    assert "colour" in _state(lambda: bctx.forward_y(y))
    bctx.set_model(*random_model(3, 3))
    _state(lambda: bctx.forward_color(synth_color(40, 30)))


def test_layers_from_per_filter_calls_are_refused(bctx, weights_blob):
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    y = synth_luma(40, 30, frame=1)
    # the per-filter calls on host planes ignore the mode, as they ignore every mode
    bctx.conv99x11(y, [np.empty(y.shape, np.float32) for _ in range(32)], w1, b1, w2, b2)
    bctx.conv55([np.ones(y.shape, np.float32)] * 32, np.empty(y.shape, np.uint8), w3, b3)
    assert "per-filter" in _state(lambda: bctx.forward_y(y))
    bctx.set_mode(S.MODE_MFMA)
    bctx.forward_y(y)                            # a complete model from per-filter calls runs on the strip path
    bctx.set_mode(S.MODE_BANDED16)
    bctx.set_weights(w1, b1, w2, b2, w3, b3)
    check(*run(bctx, y), torch_forward(y, (w1, b1, w2, b2, w3, b3)))
