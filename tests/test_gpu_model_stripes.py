"""Row stripes of every 1-channel model on the GPU (srcnn_model_rows_dev, srcnn_model_rows_halo_dev, srcnn_model_striped*): the
9-3-5 and 9-5-5 models, zero padding and SRCNN_MODE_BANDED16.  Stripes equal the whole plane bit for bit, meet the float64
restatements computed from only the rows they need, read nothing outside the rows the contract names, and the 9-1-5 model on
the strip path is forwarded to its own stripe calls.

Shapes: 200 x 61 (partial 128-column layer-1 tiles and 64-column layer-2 tiles; row ranges that are multiples of neither 8 nor
16) and 131 columns for the halo form and the striped step."""
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from color_reference import random_color_model
from spatial_reference import assert_u8_consistent, pre_tolerance, random_model, torch_forward_rows
from zero_pad_reference import torch_forward_zero_rows

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

W, H = 200, 61
RANGES = [(0, 9), (9, 10), (10, 37), (37, 61)]   # a one-row range, layer-1 row counts that are no multiple of 8, an interior range
MODES = {"mfma": S.MODE_MFMA, "banded16": S.MODE_BANDED16}
# (f2, padding, mode): f2 = 1 runs banded under zero padding, and in BANDED16 under either
CASES = [(f2, p, m) for f2, p in [(1, "zero"), (3, "replicate"), (3, "zero"), (5, "replicate"), (5, "zero")] for m in MODES]
CASES.append((1, "replicate", "banded16"))
SEED = 31


@pytest.fixture(scope="module")
def sctx():
    ctx = S.Context(0)
    yield ctx
    ctx.set_mode(S.MODE_MFMA)
    ctx.close()


def load(ctx, f2, padding, mode):
    ctx.set_mode(MODES[mode])
    ctx.set_padding(padding)
    ctx.set_model(*random_model(f2, SEED))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embedded(a, stride, fill, guard=12):
    """a [rows, w] inside a larger device tensor of row stride `stride` whose other elements (guard rows above and below, the
    columns beyond w) hold `fill`; returns (the tensor, the address of a[0, 0])."""
    rows, w = a.shape
    big = np.full((rows + 2 * guard, stride), fill, a.dtype)
    big[guard:guard + rows, :w] = a
    t = dev(big)
    return t, t.data_ptr() + guard * stride * a.itemsize


def whole_plane(ctx, y):
    h, w = y.shape
    src, dst, pre = dev(y), torch.zeros((h, w), dtype=torch.uint8, device="cuda"), torch.zeros((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.forward_y_dev(src.data_ptr(), w, 0, dst.data_ptr(), w, 0, w, h, 1, pre.data_ptr())
    ctx.synchronize()
    return dst.cpu().numpy(), pre.cpu().numpy()


def stripes(ctx, y, form="plain", fill=0, with_pre=True):
    """The plane assembled from RANGES.  plain: each range from a buffer that holds exactly [max(0, rb - R), min(h, re + R)).
    halo: d_src holds [rb, re) only, the R rows either side sit in tensors of their own with another row stride, null at the
    image edges.  Every buffer is embedded in a larger one filled with `fill`."""
    h, w = y.shape
    R = ctx.model_halo_rows()
    out, pre = np.zeros((h, w), np.uint8), np.zeros((h, w), np.float32)
    for rb, re in RANGES:
        keep = []
        d_out = torch.zeros((re - rb, w), dtype=torch.uint8, device="cuda")
        d_pre = torch.zeros((re - rb, w), dtype=torch.float32, device="cuda")
        p_pre = d_pre.data_ptr() if with_pre else 0
        if form == "plain":
            a, b = max(0, rb - R), min(h, re + R)
            t, p = embedded(y[a:b], w + 8, fill)
            keep.append(t)
            torch.cuda.synchronize()
            ctx.model_rows_dev(p, w + 8, a, d_out.data_ptr(), w, rb, w, h, rb, re, p_pre)
        else:
            t, p = embedded(y[rb:re], w + 8, fill)
            p_top = p_bot = 0
            if rb > 0:
                tt, p_top = embedded(y[rb - R:rb], w + 24, fill)
                keep.append(tt)
            if re < h:
                tb, p_bot = embedded(y[re:min(h, re + R)], w + 24, fill)
                keep.append(tb)
            keep.append(t)
            torch.cuda.synchronize()
            ctx.model_rows_halo_dev(p, w + 8, rb, re - rb, p_top, p_bot, w + 24, d_out.data_ptr(), w, rb, w, h, rb, re, p_pre)
        ctx.synchronize()
        out[rb:re], pre[rb:re] = d_out.cpu().numpy(), d_pre.cpu().numpy()
    return out, pre


_cache = {}


def results(ctx, case):
    """(y, whole (out, pre), stripes (out, pre)) of a case, computed once and shared by the tests below."""
    if case not in _cache:
        load(ctx, *case)
        y = synth_luma(W, H, frame=case[0])
        _cache[case] = (y, whole_plane(ctx, y), stripes(ctx, y))
    else:
        load(ctx, *case)
    return _cache[case]


_refs = {}


def reference_rows(f2, padding, y):
    """The float64 value before truncation of every range, each from only the input rows it needs (shared by both modes)."""
    key = (f2, padding)
    if key not in _refs:
        fn = torch_forward_rows if padding == "replicate" else torch_forward_zero_rows
        _refs[key] = [fn(y, random_model(f2, SEED), rb, re) for rb, re in RANGES]
    return _refs[key]


# ---- 1. stripes equal the whole plane, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"9-{c[0]}-5-{c[1]}-{c[2]}")
def test_stripes_equal_the_whole_plane_bit_for_bit(sctx, case):
    _, (w_out, w_pre), (s_out, s_pre) = results(sctx, case)
    assert sctx.model_halo_rows() == 6 + (case[0] - 1) // 2
    assert np.array_equal(s_out, w_out)
    assert np.array_equal(s_pre, w_pre)


# ---- 2. an independent reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"9-{c[0]}-5-{c[1]}-{c[2]}")
def test_stripes_meet_the_float64_reference_of_their_rows(sctx, case):
    y, _, (s_out, s_pre) = results(sctx, case)
    for (rb, re), ref in zip(RANGES, reference_rows(case[0], case[1], y)):
        tol = pre_tolerance(ref)
        err = np.abs(s_pre[rb:re].astype(np.float64) - ref).max()
        print(f"rows [{rb}, {re}): max |pre - ref| = {err:.3g} (tolerance {tol:.3g}, max |ref| {np.abs(ref).max():.4g})")
        assert err <= tol
        assert_u8_consistent(s_out[rb:re], ref, tol)


# ---- 3. the halo form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"9-{c[0]}-5-{c[1]}-{c[2]}")
def test_halo_buffers_give_the_same_bytes(sctx, case):
    y, _, (s_out, s_pre) = results(sctx, case)
    h_out, h_pre = stripes(sctx, y, form="halo")
    assert np.array_equal(h_out, s_out)
    assert np.array_equal(h_pre, s_pre)


@pytest.mark.parametrize("case", [(5, "replicate", "mfma"), (3, "zero", "banded16")], ids=lambda c: f"9-{c[0]}-5-{c[1]}-{c[2]}")
def test_halo_pointers_into_the_neighbours_stripes(sctx, case):
    """The same-device transport: the halo rows are read where they lie, in the neighbouring stripes' tensors (width 131)."""
    load(sctx, *case)
    w, h = 131, 61
    y = synth_luma(w, h, frame=7)
    whole, _ = whole_plane(sctx, y)
    R = sctx.model_halo_rows()
    cuts = [(0, 10), (10, 37), (37, 61)]
    ins = [dev(y[a:b]) for a, b in cuts]
    outs = [torch.zeros((b - a, w), dtype=torch.uint8, device="cuda") for a, b in cuts]
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(cuts):
        top = ins[k - 1].data_ptr() + (cuts[k - 1][1] - cuts[k - 1][0] - R) * w if k > 0 else 0
        bot = ins[k + 1].data_ptr() if k < 2 else 0
        sctx.model_rows_halo_dev(ins[k].data_ptr(), w, a, b - a, top, bot, w, outs[k].data_ptr(), w, a, w, h, a, b)
    sctx.synchronize()
    assert np.array_equal(np.concatenate([t.cpu().numpy() for t in outs]), whole)


# ---- 4. nothing outside the contract is used ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "halo"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"9-{c[0]}-5-{c[1]}-{c[2]}")
def test_rows_outside_the_contract_do_not_reach_the_output(sctx, case, form):
    """The rows and columns just outside the required buffers hold 0 in one run and 255 in the other."""
    y, _, (s_out, s_pre) = results(sctx, case)
    o_out, o_pre = stripes(sctx, y, form=form, fill=255)
    assert np.array_equal(o_out, s_out)
    assert np.array_equal(o_pre, s_pre)


# ---- 5. striped over contexts -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_pool():
    ctxs = [S.Context(0) for _ in range(3)]
    yield ctxs
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"9-{c[0]}-5-{c[1]}-{c[2]}")
def test_striped_over_contexts_equals_one_context(sctx, ctx_pool, case):
    load(sctx, *case)
    for c in ctx_pool:
        load(c, *case)
    R = sctx.model_halo_rows()
    for w, h in [(W, H), (131, 3 * R)]:          # 3 R rows over 3 contexts: a stripe's whole content is its neighbours' halo
        planes = [synth_luma(w, h, frame=f) for f in (4, 5)]
        want = [sctx.forward_y(y) for y in planes]
        for n_ctx in (2, 3):
            ctxs = ctx_pool[:n_ctx]
            for y, ref in zip(planes, want):     # the second plane reuses the buffers of the first
                assert np.array_equal(S.model_striped(ctxs, y), ref), (w, h, n_ctx)
            assert [c.halo_transport() for c in ctxs] == [1] * n_ctx
            rows = [S.stripe_rows(h, n_ctx, k) for k in range(n_ctx)]
            for y, ref in zip(planes, want):
                ins = [dev(y[a:b]) for a, b in rows]
                outs = [torch.zeros_like(t) for t in ins]
                torch.cuda.synchronize()
                S.model_striped_dev(ctxs, [t.data_ptr() for t in ins], w, [t.data_ptr() for t in outs], w, w, h)
                for c in ctxs:
                    c.synchronize()
                assert np.array_equal(np.concatenate([t.cpu().numpy() for t in outs]), ref), (w, h, n_ctx)


def test_striped_under_the_staged_transport(sctx):
    """A link that refuses peer access: the R halo rows either side are copied into the context's halo sets on a second stream.
    Forced in a fresh process by the tuning library's knob; same bytes over back-to-back steps, transport 3."""
    code = (
        "import sys, numpy as np, torch, zlib, srcnn_cpp_amd as S\n"
        "sys.path.insert(0, 'tests')\n"
        "from srcnn_cpp_amd.synth import synth_luma\n"
        "from spatial_reference import random_model\n"
        "S.use_library(S.tuning_library_path())      # the knob below exists in the tuning build only\n"
        "ctxs = [S.Context(0) for _ in range(3)]\n"
        "for c in ctxs:\n"
        "    c.set_padding('zero'); c.set_model(*random_model(5, 31))\n"
        "w, h = 200, 61\n"
        "rows = [S.stripe_rows(h, 3, k) for k in range(3)]\n"
        "crcs = []\n"
        "for f in range(6):\n"
        "    y = synth_luma(w, h, frame=f)\n"
        "    ins = [torch.from_numpy(np.ascontiguousarray(y[a:b])).cuda() for a, b in rows]\n"
        "    outs = [torch.zeros_like(t) for t in ins]\n"
        "    torch.cuda.synchronize()\n"
        "    S.model_striped_dev(ctxs, [t.data_ptr() for t in ins], w, [t.data_ptr() for t in outs], w, w, h)\n"
        "    [c.synchronize() for c in ctxs]\n"
        "    crcs.append(zlib.crc32(np.concatenate([t.cpu().numpy() for t in outs]).tobytes()))\n"
        "print(crcs, [c.halo_transport() for c in ctxs])\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(ROOT),
                       env=dict(os.environ, SRCNN_DEBUG_HALO_STAGED="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    load(sctx, 5, "zero", "mfma")
    want = [zlib.crc32(sctx.forward_y(synth_luma(200, 61, frame=f)).tobytes()) for f in range(6)]
    assert r.stdout.strip().startswith(str(want)), r.stdout
    assert "[3, 3, 3]" in r.stdout


# ---- 6. forwarding and refusals -----------------------------------------------------------------------------------------------
def _refused(fn, code=None):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == (S.ERR_STATE if code is None else code), str(e.value)
    return str(e.value)


def test_the_9_1_5_model_on_the_strip_path_is_forwarded(sctx, weights_blob):
    sctx.set_mode(S.MODE_MFMA)
    sctx.set_padding("replicate")
    sctx.set_weights_blob(weights_blob)
    assert sctx.model_halo_rows() == 6
    y = synth_luma(W, H, frame=2)
    src = dev(y)
    for rb, re in RANGES:
        a = torch.zeros((re - rb, W), dtype=torch.uint8, device="cuda")
        b = torch.zeros_like(a)
        torch.cuda.synchronize()
        sctx.model_rows_dev(src.data_ptr(), W, 0, a.data_ptr(), W, rb, W, H, rb, re)
        sctx.forward_y_rows_dev(src.data_ptr(), W, 0, b.data_ptr(), W, rb, W, H, rb, re)
        sctx.synchronize()
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        # that call has no pre-clamp output: a request for one is refused
        pre = torch.zeros((re - rb, W), dtype=torch.float32, device="cuda")
        assert "pre-clamp" in _refused(lambda: sctx.model_rows_dev(src.data_ptr(), W, 0, a.data_ptr(), W, rb, W, H, rb, re, pre.data_ptr()))
    assert np.array_equal(S.model_striped([sctx], y), sctx.forward_y(y))


def test_halo_rows_follow_the_model(sctx):
    sctx.set_padding("replicate")
    sctx.set_mode(S.MODE_MFMA)
    for f2, want in [(1, 6), (3, 7), (5, 8)]:
        sctx.set_model(*random_model(f2, 2))
        assert sctx.model_halo_rows() == want


def test_refusals_leave_the_context_usable(sctx, ctx_pool, weights_blob):
    y = synth_luma(W, H, frame=3)
    src, dst = dev(y), torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call = lambda ctx=sctx: ctx.model_rows_dev(src.data_ptr(), W, 0, dst.data_ptr(), W, 0, W, H, 10, 37)
    sctx.set_mode(S.MODE_MFMA)
    sctx.set_padding("replicate")
    # a colour model
    sctx.set_model(*random_color_model(3, 1))
    assert "colour model" in _refused(call)
    assert "colour model" in _refused(lambda: S.model_striped([sctx], y))
    # layers from per-filter calls
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    small = synth_luma(40, 30, frame=1)
    sctx.conv99x11(small, [np.empty(small.shape, np.float32) for _ in range(32)], w1, b1, w2, b2)
    sctx.conv55([np.ones(small.shape, np.float32)] * 32, np.empty(small.shape, np.uint8), w3, b3)
    assert "per-filter" in _refused(call)
    # a 9-5-5 model in a mode without arithmetic for it
    model = random_model(5, SEED)
    sctx.set_model(*model)
    sctx.set_mode(S.MODE_EXACT)
    assert "9-5-5" in _refused(call)
    sctx.set_mode(S.MODE_MFMA)
    # stripes thinner than the halo; input rows the buffer does not hold
    for c in ctx_pool:
        load(c, 5, "replicate", "mfma")
    _refused(lambda: S.model_striped(ctx_pool, synth_luma(W, 3 * 8 - 1, frame=1)), S.ERR_INVALID)
    _refused(lambda: sctx.model_rows_dev(src.data_ptr(), W, 5, dst.data_ptr(), W, 0, W, H, 10, 37), S.ERR_INVALID)
    _refused(lambda: sctx.model_rows_halo_dev(src.data_ptr(), W, 10, 27, 0, 0, W, dst.data_ptr(), W, 0, W, H, 10, 37), S.ERR_INVALID)
    # ... and after all of them the context runs the model
    call()
    sctx.synchronize()
    whole, _ = whole_plane(sctx, y)
    assert np.array_equal(dst.cpu().numpy()[10:37], whole[10:37])
