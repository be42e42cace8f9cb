"""Row stripes of a colour model and of float planes on the GPU (srcnn_model_color_rows*_dev, srcnn_model_rows*_f32_dev,
srcnn_model_color_striped*, srcnn_model_striped_f32*): packed 3-byte pixels, one float plane and three float planes, f2 = 1, 3, 5,
both paddings, SRCNN_MODE_MFMA and SRCNN_MODE_BANDED16.  Stripes equal the whole-image call bit for bit, read nothing outside
the rows and columns the contract names, meet the float64 restatements computed from only the rows they need, run striped over
contexts, and the refusals leave the context usable.

Shapes: 200 x 61 (a partial 128-column layer-1 tile and partial 64-column layer-2 tiles; a one-row range, layer-1 row counts
that are no multiple of 8, both image edges), 131 x 61 for the halo form and the striped step (one column tile plus 3), and
5 x 17 (narrower than the 9-tap window: every column is clamped or zeroed)."""
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
from color_reference import random_color_model, synth_color, torch_forward_color_rows
from spatial_reference import assert_u8_consistent, pre_tolerance, random_model, torch_forward_rows
from zero_pad_reference import torch_forward_zero_rows

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

W, H = 200, 61
RANGES = [(0, 9), (9, 10), (10, 37), (37, 61)]
SMALL = (5, 17, [(0, 8), (8, 9), (9, 17)])
MODES = {"mfma": S.MODE_MFMA, "banded16": S.MODE_BANDED16}
OTHER_MODES = [S.MODE_EXACT, S.MODE_SPLIT16, S.MODE_REFBYTES, S.MODE_REFBYTES16]
KINDS = {"color": (3, np.uint8), "f32x1": (1, np.float32), "f32x3": (3, np.float32)}     # channels, element type
# (kind, f2, padding, mode, data).  data "u8": 0..255-valued (floats: at the default input range); "unit": synth / 255 with the
# model as it is and srcnn_set_input_range(1) -- the second run of the float cases in BANDED16, the only mode that reads the range
CASES = [(k, f2, p, m, "u8") for k in KINDS for f2 in (1, 3, 5) for p in ("replicate", "zero") for m in MODES]
CASES += [(k, f2, p, "banded16", "unit") for k in ("f32x1", "f32x3") for f2 in (1, 3, 5) for p in ("replicate", "zero")]
SEED = 31
case_id = lambda c: f"{c[0]}-9-{c[1]}-5-{c[2]}-{c[3]}-{c[4]}"


@pytest.fixture(scope="module")
def sctx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx_pool():
    ctxs = [S.Context(0) for _ in range(3)]
    yield ctxs
    for c in ctxs:
        c.close()


def model_of(kind, f2, seed=SEED):
    return random_color_model(f2, seed) if KINDS[kind][0] == 3 else random_model(f2, seed)


def load(ctx, case, seed=SEED):
    kind, f2, padding, mode, data = case
    ctx.set_mode(MODES[mode])
    ctx.set_padding(padding)
    ctx.set_input_range(1.0 if data == "unit" else 255.0)
    ctx.set_model(*model_of(kind, f2, seed))


def image(kind, w, h, data="u8", frame=0):
    """The test image as [planes, h, row]: one plane of rows of 3 w bytes (packed pixels), or C planes of rows of w floats."""
    if kind == "color":
        return synth_color(w, h, frame=frame).reshape(1, h, 3 * w)
    x = synth_color(w, h, frame=frame) if kind == "f32x3" else synth_luma(w, h, frame=frame)[:, :, None]
    x = np.ascontiguousarray(np.moveaxis(x, 2, 0)).astype(np.float32)
    return x / np.float32(255.0) if data == "unit" else x


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embedded(a, stride, fill, guard):
    """a [planes, rows, row] inside a larger device tensor [planes, rows + 2 guard, stride] whose other elements (guard rows above
    and below every plane, the columns beyond the row) hold `fill`; returns (the tensor, the address of a[0, 0, 0], the channel
    pitch in elements)."""
    planes, rows, row = a.shape
    big = np.full((planes, rows + 2 * guard, stride), fill, a.dtype)
    big[:, guard:guard + rows, :row] = a
    t = dev(big)
    return t, t.data_ptr() + guard * stride * a.itemsize, (rows + 2 * guard) * stride


def halo_buffer(a, R, stride, fill, guard=5):
    """The up to R rows a [planes, rows, row] of a halo buffer inside a device tensor [planes, R + 2 guard, stride] of `fill`
    (rows the image does not hold stay `fill`): every halo buffer of a call has the channel pitch (R + 2 guard) * stride."""
    planes, rows, row = a.shape
    big = np.full((planes, R + 2 * guard, stride), fill, a.dtype)
    big[:, guard:guard + rows, :row] = a
    t = dev(big)
    return t, t.data_ptr() + guard * stride * a.itemsize


def whole_image(ctx, kind, a):
    """The whole-image call of the kind: (output [planes, h, row], pre-clamp floats or None)."""
    planes, h, row = a.shape
    src = dev(a)
    dst = torch.zeros(a.shape, dtype=src.dtype, device="cuda")
    torch.cuda.synchronize()
    if kind == "color":
        pre = torch.zeros(a.shape, dtype=torch.float32, device="cuda")
        ctx.forward_color_dev(src.data_ptr(), row, 0, dst.data_ptr(), row, 0, row // 3, h, 1, pre.data_ptr())
        ctx.synchronize()
        return dst.cpu().numpy(), pre.cpu().numpy()
    ctx.forward_f32_dev(src.data_ptr(), row, h * row, 0, dst.data_ptr(), row, h * row, 0, row, h, 1)
    ctx.synchronize()
    return dst.cpu().numpy(), None


def stripes(ctx, kind, a, ranges, form="plain", fill=None):
    """The image assembled from `ranges`.  plain: each range from a buffer that holds exactly [max(0, rb - R), min(h, re + R)).
    halo: d_src holds [rb, re) only, the R rows either side sit in tensors of their own with another row stride and another
    channel pitch, null at the image edges.  Every buffer is embedded in a larger one whose other elements hold `fill` (NaN for
    floats, 0 for bytes by default)."""
    planes, h, row = a.shape
    color = kind == "color"
    w = row // 3 if color else row
    if fill is None:
        fill = 0 if color else np.nan
    R = ctx.model_halo_rows()
    out = np.zeros(a.shape, a.dtype)
    pre = np.zeros(a.shape, np.float32) if color else None
    for rb, re in ranges:
        keep = []
        d_out = torch.zeros((planes, re - rb, row), dtype=torch.uint8 if color else torch.float32, device="cuda")
        d_pre = torch.zeros((1, re - rb, row), dtype=torch.float32, device="cuda")
        ocp = (re - rb) * row
        if form == "plain":
            lo, hi = max(0, rb - R), min(h, re + R)
            t, p, cp = embedded(a[:, lo:hi], row + 8, fill, 12)
            keep.append(t)
            torch.cuda.synchronize()
            if color:
                ctx.model_color_rows_dev(p, row + 8, lo, d_out.data_ptr(), row, rb, w, h, rb, re, d_pre.data_ptr())
            else:
                ctx.model_rows_f32_dev(p, row + 8, cp, lo, d_out.data_ptr(), row, ocp, rb, w, h, rb, re)
        else:
            t, p, cp = embedded(a[:, rb:re], row + 8, fill, 12)
            p_top = p_bot = 0
            hcp = (R + 10) * (row + 24)
            if rb > 0:
                tt, p_top = halo_buffer(a[:, rb - R:rb], R, row + 24, fill)
                keep.append(tt)
            if re < h:
                tb, p_bot = halo_buffer(a[:, re:min(h, re + R)], R, row + 24, fill)
                keep.append(tb)
            keep.append(t)
            torch.cuda.synchronize()
            if color:
                ctx.model_color_rows_halo_dev(p, row + 8, rb, re - rb, p_top, p_bot, row + 24, d_out.data_ptr(), row, rb, w, h, rb, re,
                                              d_pre.data_ptr())
            else:
                ctx.model_rows_halo_f32_dev(p, row + 8, cp, rb, re - rb, p_top, p_bot, row + 24, hcp, d_out.data_ptr(), row, ocp, rb,
                                            w, h, rb, re)
        ctx.synchronize()
        out[:, rb:re] = d_out.cpu().numpy()
        if color:
            pre[:, rb:re] = d_pre.cpu().numpy()
    return out, pre


def same(got, want):
    """bit for bit: bytes, or the bits of floats (which must be finite)"""
    if want is None:
        return got is None
    if got.dtype == np.float32:
        return bool(np.isfinite(got).all()) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return np.array_equal(got, want)


_cache = {}


def results(ctx, case):
    """(image, whole (out, pre), plain stripes (out, pre)) of a case at 200 x 61, computed once and shared by the tests below."""
    load(ctx, case)
    if case not in _cache:
        a = image(case[0], W, H, case[4], frame=case[1])
        _cache[case] = (a, whole_image(ctx, case[0], a), stripes(ctx, case[0], a, RANGES))
    return _cache[case]


# ---- 1. stripes equal the whole image, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stripes_equal_the_whole_image_bit_for_bit(sctx, case):
    a, (w_out, w_pre), (s_out, s_pre) = results(sctx, case)
    assert sctx.model_halo_rows() == 6 + (case[1] - 1) // 2
    assert same(s_out, w_out) and same(s_pre, w_pre)
    h_out, h_pre = stripes(sctx, case[0], a, RANGES, form="halo")
    assert same(h_out, w_out) and same(h_pre, w_pre)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_halo_form_at_one_column_tile_plus_three_and_narrow_images(sctx, case):
    load(sctx, case)
    kind = case[0]
    a = image(kind, 131, 61, case[4], frame=7)
    want = whole_image(sctx, kind, a)
    got = stripes(sctx, kind, a, [(0, 10), (10, 37), (37, 61)], form="halo")
    assert same(got[0], want[0]) and same(got[1], want[1])
    w, h, ranges = SMALL                       # narrower than the 9-tap window
    a = image(kind, w, h, case[4], frame=3)
    want = whole_image(sctx, kind, a)
    for form in ("plain", "halo"):
        got = stripes(sctx, kind, a, ranges, form=form)
        assert same(got[0], want[0]) and same(got[1], want[1]), form


# ---- 2. nothing outside the contract is read ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "halo"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_nothing_outside_the_contract_reaches_the_output(sctx, case, form):
    """Every buffer holds exactly the rows the contract names, inside a larger allocation: guard rows above and below each
    plane, padding columns beyond each row.  Bytes: the guard holds 0 in one run and 255 in the other, and both results are
    identical.  Floats: the guard holds NaN, and the result is finite and equal to the whole-image result."""
    a, (w_out, w_pre), _ = results(sctx, case)
    if case[0] == "color":
        lo, hi = (stripes(sctx, "color", a, RANGES, form=form, fill=f) for f in (0, 255))
        assert same(lo[0], hi[0]) and same(lo[1], hi[1])
        assert same(hi[0], w_out) and same(hi[1], w_pre)
    else:
        out, _ = stripes(sctx, case[0], a, RANGES, form=form, fill=np.nan)
        assert np.isfinite(out).all()
        assert same(out, w_out)


# ---- 3. against float64, from only the rows each range needs -----------------------------------------------------------------
_refs = {}


def reference_rows(kind, f2, padding, data, a):
    """The float64 value before truncation of every range [planes, rows, row], each from only the input rows it needs (shared
    by both modes; integer-valued float planes of 3 channels share the colour bytes' reference)."""
    channels = KINDS[kind][0]
    key = (channels, f2, padding, data)
    if key not in _refs:
        model = model_of(kind, f2)
        refs = []
        for rb, re in RANGES:
            if channels == 3:
                img = a.reshape(H, W, 3) if kind == "color" else np.moveaxis(a, 0, 2)
                refs.append(torch_forward_color_rows(np.asarray(img, np.float64), model, rb, re, padding))       # [rows, W, 3]
            else:
                fn = torch_forward_rows if padding == "replicate" else torch_forward_zero_rows
                refs.append(fn(a[0].astype(np.float64), model, rb, re)[:, :, None])
        _refs[key] = refs
    # in the layout of the kind: packed pixels, or planes
    return [r.reshape(1, r.shape[0], -1) if kind == "color" else np.moveaxis(r, 2, 0) for r in _refs[key]]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stripes_meet_the_float64_reference_of_their_rows(sctx, case):
    kind, f2, padding, _, data = case
    a, _, (s_out, s_pre) = results(sctx, case)
    r = 1.0 if data == "unit" else 255.0
    for (rb, re), ref in zip(RANGES, reference_rows(kind, f2, padding, data, a)):
        tol = pre_tolerance(ref * 255.0 / r) * r / 255.0          # for bytes (r = 255): pre_tolerance(ref)
        got = (s_pre if kind == "color" else s_out)[:, rb:re]
        err = np.abs(got.astype(np.float64) - ref).max()
        print(f"rows [{rb}, {re}): max |value - ref| = {err:.3g} (tolerance {tol:.3g}, max |ref| {np.abs(ref).max():.4g})")
        assert err <= tol
        if kind == "color":
            assert_u8_consistent(s_out[:, rb:re], ref, tol)


# ---- 4. striped over contexts ------------------------------------------------------------------------------------------------
def striped_dev(ctxs, kind, a):
    """The device-resident striped step on the rows stripe_rows() gives each context; floats: one channel pitch for all stripes."""
    planes, h, row = a.shape
    n = len(ctxs)
    rows = [S.stripe_rows(h, n, k) for k in range(n)]
    tall = max(b - lo for lo, b in rows)
    ins, outs = [], []
    for lo, b in rows:
        buf = np.zeros((planes, tall, row), a.dtype)
        buf[:, :b - lo] = a[:, lo:b]
        ins.append(dev(buf))
        outs.append(torch.zeros_like(ins[-1]))
    torch.cuda.synchronize()
    if kind == "color":
        S.model_color_striped_dev(ctxs, [t.data_ptr() for t in ins], row, [t.data_ptr() for t in outs], row, row // 3, h)
    else:
        S.model_striped_f32_dev(ctxs, [t.data_ptr() for t in ins], row, tall * row, [t.data_ptr() for t in outs], row, tall * row,
                                row, h)
    for c in ctxs:
        c.synchronize()
    return np.concatenate([t.cpu().numpy()[:, :b - lo] for t, (lo, b) in zip(outs, rows)], axis=1)


def striped_host(ctxs, kind, a):
    planes, h, row = a.shape
    if kind == "color":
        return S.model_color_striped(ctxs, a.reshape(h, row // 3, 3)).reshape(a.shape)
    if kind == "f32x1":
        return S.model_striped_f32(ctxs, a[0])[None]
    parent = np.full((planes, h + 3, row + 5), np.nan, np.float32)      # any row / channel stride
    parent[:, :h, :row] = a
    return S.model_striped_f32(ctxs, parent[:, :h, :row])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_striped_over_contexts_equals_the_whole_image(sctx, ctx_pool, case):
    load(sctx, case)
    for c in ctx_pool:
        load(c, case)
    kind = case[0]
    w, h = 131, 61                                  # 61 / 3 = 20 >= R = 8
    images = [image(kind, w, h, case[4], frame=f) for f in (4, 5)]
    want = [whole_image(sctx, kind, a)[0] for a in images]
    for n_ctx in (1, 2, 3):
        ctxs = ctx_pool[:n_ctx]
        for a, ref in zip(images, want):            # the second image reuses the buffers of the first
            assert same(striped_host(ctxs, kind, a), ref), ("host", n_ctx)
            assert same(striped_dev(ctxs, kind, a), ref), ("dev", n_ctx)
        if n_ctx > 1:
            assert [c.halo_transport() for c in ctxs] == [1] * n_ctx


def test_striped_under_the_staged_transport(sctx):
    """A link that refuses peer access: the R halo rows either side are copied, channel by channel, into the context's halo
    sets on a second stream.  Forced in a fresh process by the tuning library's knob (it is read once per process); the same
    bits over back-to-back steps, transport 3, for three float planes and for packed pixels."""
    code = (
        "import sys, numpy as np, torch, zlib, srcnn_cpp_amd as S\n"
        "sys.path.insert(0, 'tests')\n"
        "from color_reference import random_color_model, synth_color\n"
        "S.use_library(S.tuning_library_path())      # the knob below exists in the tuning build only\n"
        "ctxs = [S.Context(0) for _ in range(3)]\n"
        "for c in ctxs:\n"
        "    c.set_padding('zero'); c.set_model(*random_color_model(5, 31))\n"
        "w, h = 131, 61\n"
        "rows = [S.stripe_rows(h, 3, k) for k in range(3)]\n"
        "tall = max(b - a for a, b in rows)\n"
        "crcs = []\n"
        "for f in range(3):\n"
        "    img = synth_color(w, h, frame=f)\n"
        "    x = np.ascontiguousarray(np.moveaxis(img, 2, 0)).astype(np.float32)\n"
        "    ins = [torch.zeros((3, tall, w), dtype=torch.float32, device='cuda') for _ in rows]\n"
        "    for t, (a, b) in zip(ins, rows):\n"
        "        t[:, :b - a] = torch.from_numpy(x[:, a:b]).cuda()\n"
        "    outs = [torch.zeros_like(t) for t in ins]\n"
        "    torch.cuda.synchronize()\n"
        "    S.model_striped_f32_dev(ctxs, [t.data_ptr() for t in ins], w, tall * w, [t.data_ptr() for t in outs], w, tall * w, w, h)\n"
        "    [c.synchronize() for c in ctxs]\n"
        "    crcs.append(zlib.crc32(np.concatenate([t.cpu().numpy()[:, :b - a] for t, (a, b) in zip(outs, rows)], axis=1).tobytes()))\n"
        "    crcs.append(zlib.crc32(S.model_color_striped(ctxs, img).tobytes()))\n"
        "print(crcs, [c.halo_transport() for c in ctxs])\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(ROOT),
                       env=dict(os.environ, SRCNN_DEBUG_HALO_STAGED="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    load(sctx, ("color", 5, "zero", "mfma", "u8"))
    want = []
    for f in range(3):
        want.append(zlib.crc32(whole_image(sctx, "f32x3", image("f32x3", 131, 61, frame=f))[0].tobytes()))
        want.append(zlib.crc32(whole_image(sctx, "color", image("color", 131, 61, frame=f))[0].tobytes()))
    assert r.stdout.strip().startswith(str(want)), r.stdout
    assert "[3, 3, 3]" in r.stdout


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _refused(fn, code=None):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == (S.ERR_STATE if code is None else code), str(e.value)
    return str(e.value)


def test_refusals_leave_the_context_usable(sctx, ctx_pool, weights_blob):
    img = image("color", W, H, frame=3)
    x3 = image("f32x3", W, H, frame=3)
    src, dst = dev(img), torch.zeros((1, H, 3 * W), dtype=torch.uint8, device="cuda")
    fsrc, fdst = dev(x3), torch.zeros((3, H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    color_call = lambda ctx=sctx: ctx.model_color_rows_dev(src.data_ptr(), 3 * W, 0, dst.data_ptr(), 3 * W, 0, W, H, 10, 37)
    f32_call = lambda ctx=sctx: ctx.model_rows_f32_dev(fsrc.data_ptr(), W, H * W, 0, fdst.data_ptr(), W, H * W, 0, W, H, 10, 37)
    color_case, f32_case = ("color", 5, "replicate", "mfma", "u8"), ("f32x3", 5, "replicate", "mfma", "u8")

    def still_runs():
        """after a refusal a valid call on the same context succeeds, and gives the whole image's rows"""
        load(sctx, color_case)
        color_call()
        sctx.synchronize()
        assert same(dst.cpu().numpy()[:, 10:37], whole_image(sctx, "color", img)[0][:, 10:37])
        f32_call()
        sctx.synchronize()
        assert same(fdst.cpu().numpy()[:, 10:37], whole_image(sctx, "f32x3", x3)[0][:, 10:37])

    # the colour calls with a 1-channel model loaded
    load(sctx, ("f32x1", 3, "replicate", "mfma", "u8"))
    assert "colour model only" in _refused(color_call)
    assert "colour model only" in _refused(lambda: S.model_color_striped([sctx], img.reshape(H, W, 3)))
    halo = lambda: sctx.model_color_rows_halo_dev(src.data_ptr(), 3 * W, 0, H, 0, 0, 3 * W, dst.data_ptr(), 3 * W, 0, W, H, 10, 37)
    assert "colour model only" in _refused(halo)
    ins, outs = [src.data_ptr()], [dst.data_ptr()]
    assert "colour model only" in _refused(lambda: S.model_color_striped_dev([sctx], ins, 3 * W, outs, 3 * W, W, H))
    still_runs()
    # every mode other than MFMA / BANDED16, for the colour and for the float calls
    for mode in OTHER_MODES:
        load(sctx, color_case)
        sctx.set_mode(mode)
        _refused(color_call)
        _refused(f32_call)
        _refused(lambda: S.model_striped_f32([sctx], x3))
        load(sctx, ("f32x1", 1, "replicate", "mfma", "u8"))
        sctx.set_mode(mode)
        one = lambda: sctx.model_rows_f32_dev(fsrc.data_ptr(), W, 0, 0, fdst.data_ptr(), W, 0, 0, W, H, 10, 37)
        assert "SRCNN_MODE_MFMA and SRCNN_MODE_BANDED16 only" in _refused(one)
        still_runs()
    # layers from per-filter calls
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    small = synth_luma(40, 30, frame=1)
    sctx.conv99x11(small, [np.empty(small.shape, np.float32) for _ in range(32)], w1, b1, w2, b2)
    sctx.conv55([np.ones(small.shape, np.float32)] * 32, np.empty(small.shape, np.uint8), w3, b3)
    assert "per-filter" in _refused(lambda: sctx.model_rows_f32_dev(fsrc.data_ptr(), W, 0, 0, fdst.data_ptr(), W, 0, 0, W, H, 10, 37))
    _refused(color_call)
    still_runs()
    # stripes thinner than R = 8; contexts with different models
    for c in ctx_pool:
        load(c, color_case)
    _refused(lambda: S.model_color_striped(ctx_pool, synth_color(W, 3 * 8 - 1, frame=1)), S.ERR_INVALID)
    load(ctx_pool[1], ("color", 3, "replicate", "mfma", "u8"))
    assert "different models" in _refused(lambda: S.model_color_striped(ctx_pool, img.reshape(H, W, 3)), S.ERR_INVALID)
    load(ctx_pool[1], color_case, seed=SEED + 1)                 # the same shape, other weights
    assert "different models" in _refused(lambda: S.model_color_striped(ctx_pool, img.reshape(H, W, 3)), S.ERR_INVALID)
    for c in ctx_pool:
        load(c, f32_case)
    _refused(lambda: S.model_striped_f32(ctx_pool, np.zeros((3, 3 * 8 - 1, W), np.float32)), S.ERR_INVALID)
    ctx_pool[2].set_padding("zero")
    assert "different models" in _refused(lambda: S.model_striped_f32(ctx_pool, x3), S.ERR_INVALID)
    ctx_pool[2].set_padding("replicate")
    ctx_pool[2].set_input_range(1.0)
    assert "different models" in _refused(lambda: S.model_striped_f32(ctx_pool, x3), S.ERR_INVALID)
    ctx_pool[2].set_input_range(255.0)
    assert same(S.model_striped_f32(ctx_pool, x3), whole_image(ctx_pool[0], "f32x3", x3)[0])
    # a d_src that starts below the needed row; a missing halo buffer where the range needs one; overlapping float outputs
    load(sctx, color_case)
    _refused(lambda: sctx.model_color_rows_dev(src.data_ptr(), 3 * W, 5, dst.data_ptr(), 3 * W, 0, W, H, 10, 37), S.ERR_INVALID)
    _refused(lambda: sctx.model_color_rows_halo_dev(src.data_ptr(), 3 * W, 10, 27, 0, 0, 3 * W, dst.data_ptr(), 3 * W, 0, W, H, 10, 37),
             S.ERR_INVALID)
    _refused(lambda: sctx.model_color_rows_halo_dev(src.data_ptr(), 3 * W, 10, 27, src.data_ptr(), 0, 3 * W, dst.data_ptr(), 3 * W,
                                                    0, W, H, 10, 37), S.ERR_INVALID)
    load(sctx, f32_case)
    _refused(lambda: sctx.model_rows_f32_dev(fsrc.data_ptr(), W, H * W, 5, fdst.data_ptr(), W, H * W, 0, W, H, 10, 37), S.ERR_INVALID)
    _refused(lambda: sctx.model_rows_halo_f32_dev(fsrc.data_ptr(), W, H * W, 10, 27, 0, 0, W, 0, fdst.data_ptr(), W, H * W, 0, W, H,
                                                  10, 37), S.ERR_INVALID)
    assert "overlap each other" in _refused(lambda: sctx.model_rows_f32_dev(fsrc.data_ptr(), W, H * W, 0, fdst.data_ptr(), W, W, 0, W,
                                                                            H, 10, 37), S.ERR_INVALID)
    assert "overlap the input" in _refused(lambda: sctx.model_rows_f32_dev(fsrc.data_ptr(), W, H * W, 0, fsrc.data_ptr(), W, H * W, 0,
                                                                           W, H, 10, 37), S.ERR_INVALID)
    still_runs()
    sctx.set_input_range(255.0)
