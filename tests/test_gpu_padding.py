"""Zero padding on the GPU (srcnn_set_padding(SRCNN_PAD_ZERO)): the banded path with the zero-padding kernels against a float64
F.conv2d(padding=k // 2) restatement for the 9-1-5, 9-3-5 and 9-5-5 models, row windows across band seams, a real PyTorch
module, batches and the pipeline, the refusals, and that replicate padding is untouched."""
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle
import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from spatial_reference import assert_u8_consistent, pre_tolerance, random_model
from zero_pad_reference import torch_forward_zero, torch_forward_zero_rows

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
SIZES = [(1, 1), (3, 3), (9, 5), (17, 4), (130, 67), (260, 75)]
OTHER_MODES = [S.MODE_EXACT, S.MODE_SPLIT16, S.MODE_REFBYTES, S.MODE_REFBYTES16]


@pytest.fixture(scope="module")
def pctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _zero_mfma(pctx):
    pctx.set_mode(S.MODE_MFMA)
    pctx.set_padding("zero")
    yield
    pctx.set_padding("replicate")


def run(ctx, y):
    pre = np.empty(y.shape, np.float32)
    out = ctx.forward_y(y, preclamp=pre)
    return out, pre


def check(out, pre, ref):
    tol = pre_tolerance(ref)
    assert np.abs(pre.astype(np.float64) - ref).max() <= tol
    assert_u8_consistent(out, ref, tol)


def band_seams(width, height, f2):
    """The rows where the context's row bands meet (srcnn_spatial.cpp: two maps of 384 B per pixel within 512 MiB)."""
    r2 = (f2 - 1) // 2
    cap = (512 << 20) // (4 * width) - 64 * (4 + 2 * r2) - 32 * 4
    band_max = max(16, cap // 96)
    n = (height + band_max - 1) // band_max
    band = (height + n - 1) // n
    return list(range(band, height, band))


@pytest.mark.parametrize("f2", [1, 3, 5])
def test_matches_zero_padded_float64(pctx, f2):
    model = random_model(f2, 20)
    pctx.set_model(*model)
    assert pctx.padding() == "zero"
    for w, h in SIZES + [(1920, 1080)]:
        y = synth_luma(w, h, frame=f2)
        out, pre = run(pctx, y)
        ref = torch_forward_zero(y, model)
        assert np.abs(ref).max() < 2000
        check(out, pre, ref)


@pytest.mark.parametrize("f2", [1, 5])
def test_3840x2160_row_windows_across_band_seams(pctx, f2):
    model = random_model(f2, 21)
    pctx.set_model(*model)
    y = synth_luma(3840, 2160, frame=7)
    out, pre = run(pctx, y)
    seams = band_seams(3840, 2160, f2)
    assert len(seams) >= 5
    windows = [(0, 24), (2136, 2160)] + [(s - 12, s + 12) for s in seams[:2]] + [(seams[-1] - 12, seams[-1] + 12)]
    for r0, r1 in windows:
        check(out[r0:r1], pre[r0:r1], torch_forward_zero_rows(y, model, r0, r1))


class _Srcnn(torch.nn.Module):
    """An SRCNN as PyTorch users write it: every conv padding=k // 2 with the default padding_mode "zeros", [0, 1] input."""
    def __init__(self, f2):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(1, 64, 9, padding=4)
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=f2 // 2)
        self.conv3 = torch.nn.Conv2d(32, 1, 5, padding=2)

    def forward(self, x):
        return self.conv3(torch.relu(self.conv2(torch.relu(self.conv1(x)))))


def test_pytorch_module_end_to_end(pctx):
    m = _Srcnn(5)
    w1, b1, w2, b2, w3, b3 = random_model(5, 22)          # seeded, does not saturate on synth_luma
    with torch.no_grad():
        m.conv1.weight.copy_(torch.from_numpy(w1).reshape(64, 1, 9, 9))
        m.conv1.bias.copy_(torch.from_numpy(b1) / 255)
        m.conv2.weight.copy_(torch.from_numpy(w2))
        m.conv2.bias.copy_(torch.from_numpy(b2) / 255)
        m.conv3.weight.copy_(torch.from_numpy(w3).reshape(1, 32, 5, 5))
        m.conv3.bias.fill_(b3 / 255)
    model, padding = S.model_from_module(m)
    assert padding == "zero"
    pctx.set_padding("replicate")
    pctx.set_model(*model)
    pctx.set_padding(padding)
    y = synth_luma(203, 117, frame=3)
    with torch.no_grad():
        ref = (m.double()(torch.from_numpy(y.astype(np.float64) / 255)[None, None]) * 255)[0, 0].numpy()
    assert np.abs(ref).max() < 2000
    out, pre = run(pctx, y)
    assert np.array_equal(out, np.clip(np.trunc(pre), 0, 255).astype(np.uint8))
    check(out, pre, ref)


def test_device_batch_frames_and_pipeline(pctx):
    model = random_model(3, 23)
    pctx.set_model(*model)
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
    pctx.forward_y_dev(d_src.data_ptr(), sstride, spitch, d_dst.data_ptr(), dstride, dpitch, w, h, n)
    for k in range(n):
        pctx.forward_y_dev(d_src.data_ptr() + k * spitch, sstride, 0, d_one.data_ptr() + k * dpitch, dstride, 0, w, h, 1)
    pctx.synchronize()
    batch, single = d_dst.cpu().numpy(), d_one.cpu().numpy()
    assert np.array_equal(batch, single)
    outs = [single[k * dpitch:k * dpitch + dstride * h].reshape(h, dstride)[:, :w] for k in range(n)]
    assert np.array_equal(np.stack(outs), pctx.forward_y_frames(frames))
    for k in range(n):
        assert np.array_equal(outs[k], pctx.forward_y(frames[k]))
    check(outs[1], run(pctx, frames[1])[1], torch_forward_zero(frames[1], model))

    rng = np.random.default_rng(4)
    bgr = (rng.integers(0, 256, (61, 83, 3)) // 8 * 8).astype(np.uint8)
    scale = 1.5
    ow, oh = S.scaled_size(83, 61, scale)
    planes = [pctx.resize_cubic(p, ow, oh) for p in pctx.bgr2ycrcb(bgr)]
    want = pctx.ycrcb2bgr(pctx.forward_y(planes[0]), planes[1], planes[2])
    assert np.array_equal(pctx.process_bgr(bgr, scale), want)
    d_in = torch.from_numpy(bgr).cuda()
    d_out = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pctx.process_bgr_dev(d_in.data_ptr(), 3 * 83, 83, 61, scale, d_out.data_ptr(), 3 * ow)
    pctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)


def _state(fn):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == S.ERR_STATE
    return str(e.value)


@pytest.mark.parametrize("f2", [1, 5])
def test_refusals_under_zero_padding(pctx, weights_blob, f2):
    model = random_model(f2, 24)
    pctx.set_model(*model)
    w, h = 64, 32
    y = synth_luma(w, h)
    d_src = torch.from_numpy(y).cuda()
    d_dst = torch.zeros_like(d_src)
    d_work = torch.zeros(32 * w * h, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p, o = d_src.data_ptr(), d_dst.data_ptr()
    msgs = [
        _state(lambda: pctx.forward_y_rows_dev(p, w, 0, o, w, 0, w, h, 0, h)),
        _state(lambda: pctx.forward_y_rows_halo_dev(p, w, 0, h, 0, 0, w, o, w, 0, w, h, 0, h)),
        _state(lambda: pctx.forward_y_unfused_dev(p, w, 0, o, w, 0, w, h, 1, d_work.data_ptr())),
        _state(lambda: pctx.conv99x11_dev(p, w, d_work.data_ptr(), w, w * h, w, h)),
        _state(lambda: pctx.conv55_dev(d_work.data_ptr(), w, w * h, o, w, w, h)),
        _state(lambda: S.forward_y_striped([pctx], y)),
        _state(lambda: S.forward_y_striped_frames([pctx], y[None])),
        _state(lambda: S.forward_y_frames_multi([pctx], y[None])),
        _state(lambda: S.forward_y_lanes_dev([pctx], [p], w, [o], w, w, h)),
        _state(lambda: S.forward_y_striped_dev([pctx], [p], w, [o], w, w, h)),
    ]
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    f32 = lambda: np.empty(y.shape, np.float32)
    msgs += [
        _state(lambda: pctx.conv99(y, f32(), w1[0], float(b1[0]))),
        _state(lambda: pctx.conv11([np.ones(y.shape, np.float32)] * 64, f32(), w2[0], float(b2[0]))),
        _state(lambda: pctx.conv55([np.ones(y.shape, np.float32)] * 32, np.empty(y.shape, np.uint8), w3, b3)),
        _state(lambda: pctx.conv99x11(y, [f32() for _ in range(32)], w1, b1, w2, b2)),
        _state(lambda: pctx.conv99x11_to_dev(y, d_work.data_ptr(), w, w * h, w1, b1, w2, b2)),
        _state(lambda: pctx.conv55_from_dev(d_work.data_ptr(), w, w * h, np.empty(y.shape, np.uint8), w3, b3)),
    ]
    assert all("SRCNN_PAD_ZERO" in m for m in msgs), msgs
    assert pctx.model_f2() == f2                 # the refused per-filter calls did not end the model
    for mode in OTHER_MODES:
        pctx.set_mode(mode)
        msg = _state(lambda: pctx.forward_y(y))
        assert "SRCNN_PAD_ZERO" in msg and "SRCNN_MODE_MFMA" in msg
        _state(lambda: pctx.forward_y_frames(y[None]))
        _state(lambda: pctx.process_bgr(np.zeros((16, 16, 3), np.uint8), 2.0))
    pctx.set_mode(S.MODE_MFMA)
    out, pre = run(pctx, y)                      # the context still runs the model
    check(out, pre, torch_forward_zero(y, model))
    with pytest.raises(S.SrcnnError) as e:
        pctx._check(pctx._lib.srcnn_set_padding(pctx._h, 2))
    assert e.value.code == S.ERR_INVALID
    with pytest.raises(ValueError):
        pctx.set_padding("reflect")
    assert pctx.padding() == "zero"


def test_layers_from_per_filter_calls_are_refused(pctx, weights_blob):
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    y = synth_luma(40, 30, frame=1)
    pctx.set_padding("replicate")
    pctx.conv99x11(y, [np.empty(y.shape, np.float32) for _ in range(32)], w1, b1, w2, b2)
    pctx.conv55([np.ones(y.shape, np.float32)] * 32, np.empty(y.shape, np.uint8), w3, b3)
    pctx.forward_y(y)                            # a complete model from per-filter calls runs with replicate padding
    pctx.set_padding("zero")
    assert "per-filter" in _state(lambda: pctx.forward_y(y))
    pctx.set_weights(w1, b1, w2, b2, w3, b3)
    check(*run(pctx, y), torch_forward_zero(y, (w1, b1, w2, b2, w3, b3)))


def test_padding_survives_model_loads(pctx):
    y = synth_luma(70, 41, frame=5)
    for f2 in (5, 1, 3):
        model = random_model(f2, 25)
        pctx.set_model(*model)
        assert pctx.padding() == "zero"
        check(*run(pctx, y), torch_forward_zero(y, model))


def butterfly():
    return np.fromfile(GOLD / "butterfly_y_in_576.u8", np.uint8).reshape(576, 576)


def test_replicate_round_trip_is_bit_identical(pctx, weights_blob):
    pctx.set_padding("replicate")
    pctx.set_model(*random_model(5, 26))
    y = synth_luma(300, 170, frame=2)
    before, pre_before = run(pctx, y)
    pctx.set_padding("zero")
    zero, _ = run(pctx, y)
    assert not np.array_equal(zero, before)
    pctx.set_padding("replicate")
    after, pre_after = run(pctx, y)
    assert np.array_equal(before, after) and np.array_equal(pre_before, pre_after)

    pctx.set_padding("zero")
    pctx.set_weights_blob(weights_blob)
    run(pctx, butterfly())
    pctx.set_padding("replicate")
    pctx.set_mode(S.MODE_REFBYTES)
    r_out, _ = oracle.forward_y(butterfly(), weights_blob)
    assert np.array_equal(pctx.forward_y(butterfly()), r_out)


def test_two_contexts_keep_their_own_padding(pctx):
    model = random_model(3, 27)
    y = synth_luma(150, 60, frame=6)
    pctx.set_model(*model)
    with S.Context(0) as other:
        other.set_model(*model)
        assert other.padding() == "replicate"
        rep = other.forward_y(y)
        zero, zpre = run(pctx, y)
        assert np.array_equal(other.forward_y(y), rep)
        assert pctx.padding() == "zero" and other.padding() == "replicate"
        check(zero, zpre, torch_forward_zero(y, model))
        pctx.set_padding("replicate")
        assert np.array_equal(pctx.forward_y(y), rep)
