"""The hazard-safe strip kernels (srcnn_set_kernel_variant(ctx, 1)): every instantiation launch_strip_safe() can launch, against
the CPU model of the kernels' summation order.

csrc/srcnn_mfma.hip is compiled twice; the second object (-DSRCNN_SAFE_HAZARDS=1, namespace srcnn::safe) is separate machine
code -- builtin MFMAs and a plain max where the fast form has inline asm, other registers, other scheduling, wait states the
compiler pads -- and it is what a context launches whose interlock probe disagrees or whose deployment pins it.  The comparisons
are the ones the fast form gets in test_gpu_parity.py, test_gpu_refbytes.py and test_gpu_spatial.py, under variant 1:

* the primary oracle is the model of the kernels' arithmetic (``oracle.gpuorder_*``), BITWISE;
* in the REFBYTES modes it is the reference's arithmetic (``oracle.forward_y``), BITWISE;
* where the reference arithmetic is compared as well, the tolerances are test_gpu_parity.py's (imported, none of its own);
* "equal to the fast form" is only ever an extra assertion: both forms could share a defect.

Which test launches which instantiation.  launch_strip_safe() picks it from the strip mode, a pre-clamp plane (PRE), a flag
plane (FIX: the context is in SRCNN_MODE_REFBYTES) and halo buffers (HALO3), so the entry point and the context's mode decide it;
the geometry (work items or regular grid, column seams) is asserted through query_plan in the tests that depend on it; and each
test named here failed when a value was changed in the safe translation unit alone (the ReLU under #if SRCNN_SAFE_HAZARDS for
MODE_FUSED / MODE_L12; MODE_L3 has no line of its own there, its tap partials were changed under the define):
    MODE_FUSED plain ........ test_fused_plain_and_pre, test_work_items_*, test_row_ranges_*, the batches, test_two_contexts_*
    MODE_FUSED PRE .......... test_fused_plain_and_pre, test_work_items_with_seams (d_pre), test_small_batches_*, test_random_weights
    MODE_FUSED FIX .......... test_refbytes_*, test_random_weights, test_halo_rows_* (a stripe that needs no halo)
    MODE_FUSED HALO3 ........ test_halo_rows_in_their_own_buffers[MFMA]
    MODE_FUSED HALO3 FIX .... test_halo_rows_in_their_own_buffers[REFBYTES]
    MODE_L12 ................ test_conv99x11_*, test_device_plane_call_sites, test_batch_fused_and_unfused
    MODE_L3 ................. test_conv55, test_device_plane_call_sites, test_batch_fused_and_unfused, test_byte_models_layer3 (no pre-clamp request)
    MODE_L3 PRE ............. test_conv55 (srcnn_conv55_dev with d_preclamp), test_byte_models_layer3 (pre-clamp floats out)
(MODE_FUSED DIAG=2 is the tuning build's stamped kernel and not part of the product surface.)
"""
import numpy as np
import pytest

import oracle
import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_batch, synth_luma
from spatial_reference import band_seams, random_model, torch_forward, torch_forward_rows
from test_gpu_parity import EDGE_SIZES, TILE_SIZES, TOL_MAP_REL, TOL_PRE_ABS, check_u8, planes32
from test_gpu_spatial import check as check_spatial          # pre_tolerance() + assert_u8_consistent(): that file's tolerance

pytestmark = pytest.mark.gpu

ITEM_PLANES = [(1920, 400), (3840, 601)]       # the smallest planes the fast form's tests run as work items with seams + FAST body
ITEM_FRAME = 21                                 # one synthetic frame for every test on them: one model plane each per module


@pytest.fixture(scope="module")
def safe_ctx(weights_blob):
    ctx = S.Context(0)
    ctx.set_weights_blob(weights_blob)
    ctx.set_kernel_variant(1)
    assert ctx.kernel_variant() == 1
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _still_pinned(safe_ctx):
    """A call that silently reset the variant would make the test exercise the fast form: every test ends with the pin checked."""
    assert safe_ctx.kernel_variant() == 1
    yield
    assert safe_ctx.kernel_variant() == 1, "the context lost its pin during the test: it ran the FAST kernels"


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_PLANES = {}


def plane(w, h, frame, weights_blob, reference=False):
    """(input, model bytes, model pre-clamp floats) of a synthetic plane -- or the reference arithmetic's pair -- computed once per
    module, the expected planes handed out read-only (the input stays writable: torch.from_numpy() wants that)."""
    key = (w, h, frame, reference)
    if key not in _PLANES:
        y = synth_luma(w, h, frame=frame)
        out, pre = (oracle.forward_y if reference else oracle.gpuorder_forward_y)(y, weights_blob)
        for a in (out, pre):
            a.flags.writeable = False
        _PLANES[key] = (y, out, pre)
    return _PLANES[key]


def runs_as_work_items(ctx, w, h):
    """query_plan: a plane cut into work items reports the item count (2 per CU), which is no multiple of its strip count here,
    where the regular grid reports strips x segments; and its strips are the FW = 128 column ones of the column-seam form."""
    p = ctx.query_plan(w, h, 1)
    return p["workgroups"] != p["strips"] * p["segments"] and p["strips"] == (w + 127) // 128 and p["seg_rows"] < h


# ---------------------------------------------------------------- 1. MODE_L12: Convolution99x11

@pytest.mark.parametrize("w,h", EDGE_SIZES + TILE_SIZES)
def test_conv99x11(safe_ctx, weights_blob, w, h):
    w1, b1, w2, b2, *_ = S.split_weights(weights_blob)
    y = synth_luma(w, h, frame=1)
    buf, dst = planes32(h, w)
    buf[:] = -1.0
    safe_ctx.conv99x11(y, dst, w1, b1, w2, b2)
    assert np.array_equal(buf, oracle.gpuorder_conv99x11(y, w1, b1, w2, b2)), "safe layer 1-2 differs from its FMA-order model"
    ref = oracle.conv99x11(y, w1, b1, w2, b2)
    assert (np.abs(buf - ref) <= TOL_MAP_REL * np.maximum(1.0, np.abs(ref))).all()


def test_conv99x11_strided_planes(safe_ctx, weights_blob):
    w1, b1, w2, b2, *_ = S.split_weights(weights_blob)
    ybuf = np.zeros((30, 80), np.uint8)
    ybuf[:, :71] = synth_luma(71, 30)
    y = ybuf[:, :71]
    buf, dst = planes32(30, 71, stride=96)
    buf[:] = np.float32(-5)
    safe_ctx.conv99x11(y, dst, w1, b1, w2, b2)
    assert np.array_equal(buf[:, :, :71], oracle.gpuorder_conv99x11(np.ascontiguousarray(y), w1, b1, w2, b2))
    assert (buf[:, :, 71:] == -5).all(), "wrote outside the plane's columns"


# ---------------------------------------------------------------- 2. MODE_L3: Convolution55

@pytest.mark.parametrize("w,h", EDGE_SIZES + TILE_SIZES)
def test_conv55(safe_ctx, weights_blob, w, h):
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    feat = oracle.conv99x11(synth_luma(w, h, frame=4), w1, b1, w2, b2)
    dst = np.full((h, w), 77, np.uint8)
    safe_ctx.conv55([feat[k] for k in range(32)], dst, w3, b3)
    model, model_pre = oracle.gpuorder_conv55(feat, w3, b3)
    assert np.array_equal(dst, model), "safe layer 3 differs from its FMA-order model"
    ref, ref_pre = oracle.conv55(feat, w3, b3)
    check_u8(dst, ref, ref_pre)
    # the same planes from device memory with the pre-clamp floats out (MODE_L3 with PRE): a float that is off shows on a
    # plane too small for a byte to flip
    torch = _torch()
    d_feat = torch.from_numpy(feat).cuda()
    d_dst = torch.full((h, w), 77, dtype=torch.uint8, device="cuda")
    d_pre = torch.full((h, w), -3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    safe_ctx.conv55_dev(d_feat.data_ptr(), w, w * h, d_dst.data_ptr(), w, w, h, d_pre.data_ptr())
    safe_ctx.synchronize()
    assert np.array_equal(d_pre.cpu().numpy(), model_pre), "safe layer 3 (PRE) differs from its FMA-order model (pre-clamp)"
    assert np.array_equal(d_dst.cpu().numpy(), model)
    assert np.abs(d_pre.cpu().numpy() - ref_pre).max() <= TOL_PRE_ABS


def test_device_plane_call_sites(safe_ctx, weights_blob):
    """srcnn_conv99x11_to_dev + srcnn_conv55_from_dev with the 32-plane map kept in device memory (test_gpu_hardening.py,
    test_reference_call_sites_with_device_planes), 333 x 97."""
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    w, h = 333, 97
    y = synth_luma(w, h, frame=6)
    d = safe_ctx.dev_alloc(32 * w * h * 4)
    try:
        out = np.empty_like(y)
        safe_ctx.conv99x11_to_dev(y, d, w, w * h, w1, b1, w2, b2)
        safe_ctx.conv55_from_dev(d, w, w * h, out, w3, b3)
        planes = safe_ctx.dev_download(np.empty((32, h, w), np.float32), d)
    finally:
        safe_ctx.dev_free(d)
        safe_ctx.set_weights_blob(weights_blob)
    assert np.array_equal(planes, oracle.gpuorder_conv99x11(y, w1, b1, w2, b2))
    assert np.array_equal(out, oracle.gpuorder_forward_y(y, weights_blob)[0])


# ---------------------------------------------------------------- 3. MODE_FUSED with PRE, and plain, on the regular grid

@pytest.mark.parametrize("w,h", EDGE_SIZES + TILE_SIZES)
def test_fused_plain_and_pre(safe_ctx, weights_blob, w, h):
    y = synth_luma(w, h)
    m_out, m_pre = oracle.gpuorder_forward_y(y, weights_blob)
    pre = np.full((h, w), -3.0, np.float32)
    out = safe_ctx.forward_y(y, preclamp=pre)                         # PRE
    assert np.array_equal(pre, m_pre), "safe fused kernel (PRE) differs from its FMA-order model (pre-clamp)"
    assert np.array_equal(out, m_out)
    assert np.array_equal(safe_ctx.forward_y(y), m_out), "safe fused kernel (plain) differs from its FMA-order model"
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    assert np.abs(pre - r_pre).max() <= TOL_PRE_ABS
    check_u8(out, r_out, r_pre)


@pytest.mark.parametrize("value", [0, 255])
def test_constant_planes(safe_ctx, weights_blob, value):
    y = np.full((37, 150), value, np.uint8)
    m_out, m_pre = oracle.gpuorder_forward_y(y, weights_blob)
    pre = np.empty(y.shape, np.float32)
    assert np.array_equal(safe_ctx.forward_y(y, preclamp=pre), m_out) and np.array_equal(pre, m_pre)
    out = safe_ctx.forward_y(y)
    assert np.array_equal(out, m_out)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    check_u8(out, r_out, r_pre)
    assert (out == out[0, 0]).all()


def test_saturating_input(safe_ctx, weights_blob):
    """i.i.d. bytes drive the output into the 0/255 clamp (test_gpu_parity.py, test_forward_saturating_input)."""
    y = np.random.default_rng(7).integers(0, 256, (64, 140), dtype=np.uint8)
    m_out, m_pre = oracle.gpuorder_forward_y(y, weights_blob)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    pre = np.empty(y.shape, np.float32)
    assert np.array_equal(safe_ctx.forward_y(y, preclamp=pre), m_out) and np.array_equal(pre, m_pre)
    out = safe_ctx.forward_y(y)
    assert np.array_equal(out, m_out)
    assert ((r_out == 0) | (r_out == 255)).mean() > 0.2
    check_u8(out, r_out, r_pre)


# ---------------------------------------------------------------- 4. work items, row seams, column seams, four-row body

@pytest.mark.parametrize("w,h", ITEM_PLANES)
def test_work_items_with_seams(safe_ctx, weights_blob, w, h):
    """The seam kernels live in the fast translation unit only; they read the seam scratch the SAFE strip kernel writes.  Both
    planes run as 512 work items on 256 compute units (query_plan: 512 != 15 x 35 and != 30 x 18; strips of 128 columns, i.e.
    column seams; items of at most 13 / 48 rows, i.e. row seams between the items of a strip), the steady-state rows of every
    item through the four-row FAST body.  Without a pre-clamp plane that is the plain instantiation, with one the PRE
    instantiation on the same items (general body, same seams)."""
    torch = _torch()
    assert runs_as_work_items(safe_ctx, w, h), safe_ctx.query_plan(w, h, 1)
    y, m_out, m_pre = plane(w, h, ITEM_FRAME, weights_blob)
    d_in = torch.from_numpy(y).cuda()
    d_out = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
    d_out2 = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
    d_pre = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    safe_ctx.forward_y_dev(d_in.data_ptr(), w, 0, d_out.data_ptr(), w, 0, w, h, 1)
    safe_ctx.forward_y_dev(d_in.data_ptr(), w, 0, d_out2.data_ptr(), w, 0, w, h, 1, d_pre.data_ptr())
    safe_ctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), m_out), "plain instantiation on work items"
    assert np.array_equal(d_out2.cpu().numpy(), m_out) and np.array_equal(d_pre.cpu().numpy(), m_pre), "PRE instantiation on work items"


@pytest.mark.parametrize("w,h", [(300, 97), (3840, 601)])
def test_row_ranges_of_every_alignment(safe_ctx, weights_blob, w, h):
    """The sweep of test_gpu_parity.py's test of this name, whole: every first row 0..9 against every last row h-9..h, the
    short ranges, the tall ranges on the item plane; padded output rows whose guard bytes stay."""
    torch = _torch()
    y, model, _ = plane(w, h, ITEM_FRAME, weights_blob)
    assert np.array_equal(safe_ctx.forward_y(y), model)
    d_in = torch.from_numpy(y).cuda()
    ranges = [(r0, r1) for r0 in range(0, 10) for r1 in (h, h - 1, h - 2, h - 3, h - 5, h - 9)]
    ranges += [(r0, r0 + n) for r0 in (0, 3, 14, 41) for n in (1, 2, 5, 11, 12, 13, 19, 24, 31)]
    if h > 400:
        ranges += [(r0, r0 + n) for r0 in (7, 100, 233) for n in (200, 257, 300, 366)]
    for r0, r1 in ranges:
        d_out = torch.full((r1 - r0, w + 12), 5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        safe_ctx.forward_y_rows_dev(d_in.data_ptr(), w, 0, d_out.data_ptr(), w + 12, r0, w, h, r0, r1)
        safe_ctx.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:, :w], model[r0:r1]), (r0, r1)
        assert (got[:, w:] == 5).all(), (r0, r1)    # nothing written beyond the row


# ---------------------------------------------------------------- 5. HALO3, and HALO3 with FIX

@pytest.mark.parametrize("mode", [S.MODE_MFMA, S.MODE_REFBYTES], ids=["MFMA", "REFBYTES"])
@pytest.mark.parametrize("w,h,n_stripes", [(260, 90, 3), (260, 97, 8), (3840, 601, 3)])
def test_halo_rows_in_their_own_buffers(safe_ctx, weights_blob, mode, w, h, n_stripes):
    """srcnn_forward_y_rows_halo_dev under variant 1: the rows of each stripe in an exactly sized allocation, the 6 rows of each
    neighbour in buffers with a row stride of their own (w + 20), one launch per stripe; the stitched plane is the model's in
    MODE_MFMA and the reference's in MODE_REFBYTES.  First and last stripe hold one halo buffer, the others two; then the
    sub-range that needs one halo only and the one that needs none (which is the plain / FIX instantiation)."""
    torch = _torch()
    y, want, _ = plane(w, h, ITEM_FRAME if (w, h) in ITEM_PLANES else 13, weights_blob, reference=mode == S.MODE_REFBYTES)
    hs = w + 20
    safe_ctx.set_mode(mode)
    try:
        reruns = safe_ctx.fixup_stats()["exact_reruns"]
        out = np.zeros_like(y)
        for k in range(n_stripes):
            r0, r1 = S.stripe_rows(h, n_stripes, k)
            d_own = torch.from_numpy(np.ascontiguousarray(y[r0:r1])).cuda()
            top = bot = None
            if k > 0:
                top = torch.full((6, hs), 77, dtype=torch.uint8, device="cuda")
                top[:, :w] = torch.from_numpy(np.ascontiguousarray(y[r0 - 6:r0])).cuda()
            if k < n_stripes - 1:
                bot = torch.full((6, hs), 77, dtype=torch.uint8, device="cuda")
                bot[:, :w] = torch.from_numpy(np.ascontiguousarray(y[r1:r1 + 6])).cuda()
            d_out = torch.zeros((r1 - r0, w), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            safe_ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, top.data_ptr() if top is not None else 0,
                                             bot.data_ptr() if bot is not None else 0, hs, d_out.data_ptr(), w, r0, w, h, r0, r1)
            safe_ctx.synchronize()
            out[r0:r1] = d_out.cpu().numpy()
        assert np.array_equal(out, want)
        r0, r1 = S.stripe_rows(h, n_stripes, 1)
        if r1 - r0 >= 14:
            d_own = torch.from_numpy(np.ascontiguousarray(y[r0:r1])).cuda()
            top = torch.full((6, hs), 77, dtype=torch.uint8, device="cuda")
            top[:, :w] = torch.from_numpy(np.ascontiguousarray(y[r0 - 6:r0])).cuda()
            d_one = torch.zeros((r1 - r0, w), dtype=torch.uint8, device="cuda")
            d_none = torch.zeros((r1 - r0, w), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            safe_ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, top.data_ptr(), 0, hs, d_one.data_ptr(), w, r0, w, h, r0, r1 - 6)
            safe_ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, 0, 0, hs, d_none.data_ptr(), w, r0, w, h, r0 + 6, r1 - 6)
            safe_ctx.synchronize()
            assert np.array_equal(d_one.cpu().numpy()[:r1 - r0 - 6], want[r0:r1 - 6]), "the top halo only"
            assert np.array_equal(d_none.cpu().numpy()[6:r1 - r0 - 6], want[r0 + 6:r1 - 6]), "no halo"
        else:
            assert (w, h, n_stripes) == (260, 97, 8)          # stripes of 12 rows: every launch above reads both halos
        assert safe_ctx.fixup_stats()["exact_reruns"] == reruns, "the re-run net fired: the flags did not cover the noise"
    finally:
        safe_ctx.set_mode(S.MODE_MFMA)


# ---------------------------------------------------------------- 6. FIX: SRCNN_MODE_REFBYTES

@pytest.mark.parametrize("w,h", TILE_SIZES + ITEM_PLANES)
def test_refbytes(safe_ctx, weights_blob, w, h):
    """The reference's bytes, bit for bit, from the safe FIX instantiation -- on the regular grid (tile-edge shapes) and on work
    items with seams (the item planes) -- and without the re-run net, which would hand back the reference's bytes whatever the
    strip kernel wrote."""
    if (w, h) in ITEM_PLANES:
        assert runs_as_work_items(safe_ctx, w, h)
        y, want, _ = plane(w, h, ITEM_FRAME, weights_blob, reference=True)
    else:
        y = synth_luma(w, h, frame=5)
        want = oracle.forward_y(y, weights_blob)[0]
    safe_ctx.set_mode(S.MODE_REFBYTES)
    try:
        before = safe_ctx.fixup_stats()
        got = safe_ctx.forward_y(y)
        after = safe_ctx.fixup_stats()
    finally:
        safe_ctx.set_mode(S.MODE_MFMA)
    assert np.array_equal(got, want)
    assert after["exact_reruns"] == before["exact_reruns"], "the re-run net fired"
    assert 0 <= after["max_dev"] < 0.5 * after["delta"], after


@pytest.mark.parametrize("w,h", [(300, 70)] + ITEM_PLANES)
def test_refbytes_flags_are_the_fast_forms(weights_blob, w, h):
    """The flags depend on the strip kernel's floats alone, which must be the same in both forms: after the same plane a fresh
    variant-0 context and a fresh variant-1 context report the same fix-up statistics (pixels flagged, dense tiles, bytes changed,
    largest monitored deviation, no re-run).  A safe FIX instantiation that flags differently and is rescued by the fix-up
    returns the right bytes and fails here."""
    y, want, _ = plane(w, h, ITEM_FRAME if (w, h) in ITEM_PLANES else 5, weights_blob, reference=True)
    stats = []
    for variant in (0, 1):
        with S.Context(0) as ctx:
            ctx.set_weights_blob(weights_blob)
            ctx.set_kernel_variant(variant)
            ctx.set_mode(S.MODE_REFBYTES)
            assert ctx.kernel_variant() == variant
            assert np.array_equal(ctx.forward_y(y), want), variant
            stats.append((ctx.fixup_stats(), ctx.fixup_local_stats()))
            assert ctx.kernel_variant() == variant
    assert stats[0] == stats[1], stats
    assert stats[1][0]["exact_reruns"] == 0 and stats[1][0]["scattered_pixels"] > 0


# ---------------------------------------------------------------- 7. batches

def test_batch_fused_and_unfused(safe_ctx, weights_blob):
    """Five 200 x 45 frames through the fused kernel and through MODE_L12 + MODE_L3 on a batch: both the model's bytes."""
    torch = _torch()
    n, h, w = 5, 45, 200
    frames = synth_batch(w, h, n)
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.zeros_like(d_in)
    d_out2 = torch.zeros_like(d_in)
    d_work = torch.empty((n, 32, h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    safe_ctx.forward_y_dev(d_in.data_ptr(), w, h * w, d_out.data_ptr(), w, h * w, w, h, n)
    safe_ctx.forward_y_unfused_dev(d_in.data_ptr(), w, h * w, d_out2.data_ptr(), w, h * w, w, h, n, d_work.data_ptr())
    safe_ctx.synchronize()
    a, b = d_out.cpu().numpy(), d_out2.cpu().numpy()
    for k in range(n):
        m_out, _ = oracle.gpuorder_forward_y(frames[k], weights_blob)
        assert np.array_equal(a[k], m_out), f"fused, frame {k}"
        assert np.array_equal(b[k], m_out), f"layers 1-2 + layer 3, frame {k}"


@pytest.mark.parametrize("w,h,n", [(1920, 1080, 2), (1280, 400, 3)])
def test_small_batches_repeat_the_item_plan_per_frame(safe_ctx, weights_blob, w, h, n):
    """A batch below 32 frames runs the plane's work items frame after frame: padded row strides and frame pitches, with d_pre
    (the PRE instantiation on items with seams).  query_plan: n x the single plane's items either way; 2 x 1920x1080 is queued as
    one launch per frame (frames_per_launch()), 3 x 1280x400 as ONE launch of 3 x 256 items (256 != 10 strips x 26).  Every
    frame equals the plane computed alone; one frame is compared with the model (which costs seconds per 2 MPix)."""
    torch = _torch()
    one = safe_ctx.query_plan(w, h, 1)
    assert safe_ctx.query_plan(w, h, n)["workgroups"] == n * one["workgroups"] and runs_as_work_items(safe_ctx, w, h), one
    frames = synth_batch(w, h, n, first_frame=20)
    pitch = (h + 3) * (w + 64)
    d_in = torch.zeros((n, pitch), dtype=torch.uint8, device="cuda")
    d_in[:, : h * (w + 64)].view(n, h, w + 64)[:, :, :w] = torch.from_numpy(frames).cuda()
    d_out = torch.full((n, pitch), 7, dtype=torch.uint8, device="cuda")
    d_pre = torch.zeros((n, pitch), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    safe_ctx.forward_y_dev(d_in.data_ptr(), w + 64, pitch, d_out.data_ptr(), w + 64, pitch, w, h, n, d_pre.data_ptr())
    safe_ctx.synchronize()
    got = d_out[:, : h * (w + 64)].view(n, h, w + 64).cpu().numpy()
    pre = d_pre[:, : h * (w + 64)].view(n, h, w + 64).cpu().numpy()
    assert (got[:, :, w:] == 7).all(), "wrote outside the frames' columns"
    for k in range(n):
        alone_pre = np.empty((h, w), np.float32)
        alone = safe_ctx.forward_y(frames[k], preclamp=alone_pre)
        assert np.array_equal(got[k, :, :w], alone) and np.array_equal(pre[k, :, :w], alone_pre), k
    m_out, m_pre = oracle.gpuorder_forward_y(frames[n - 1], weights_blob)
    assert np.array_equal(got[n - 1, :, :w], m_out) and np.array_equal(pre[n - 1, :, :w], m_pre)


@pytest.mark.parametrize("w,h", [(125, 9), (249, 9)])
def test_batch_on_the_regular_grid_with_column_seams(safe_ctx, weights_blob, w, h):
    """strip_geometry(): from kItemBatchMax = 32 frames on a batch runs on the regular strip x segment x frame grid, with column
    seams where cseam_pays(width): strips of 128 output columns must be fewer than strips of 124 with halo columns.  125 is the
    smallest such width (1 strip against 2) -- the branch is taken, but no seam lies between two strips; 249 is the smallest
    with one (2 strips against 3, the last 121 columns wide), whose four edge pixels per row srcnn_cseam_kernel finishes from
    what the SAFE strip kernel exported.  The height
    does not enter the decision; 9 rows leave rows whose 5 x 5 window meets neither the top nor the bottom edge.
    Confirmed with the tuning build's srcnn_debug_strip_geometry for 256 compute units (items 0, column seams 1 for both
    widths at 32 frames) and here through query_plan: strips = ceil(w / 128) -- the halo-column form would report
    ceil(w / 124) -- and workgroups = strips x segments x frames.  Every frame equals the plane computed alone, and the model."""
    torch = _torch()
    n = 32
    p = safe_ctx.query_plan(w, h, n)
    assert p["strips"] == (w + 127) // 128 < (w + 123) // 124 and p["workgroups"] == p["strips"] * p["segments"] * n, p
    frames = synth_batch(w, h, n, first_frame=40)
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.full((n, h, w + 8), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    safe_ctx.forward_y_dev(d_in.data_ptr(), w, h * w, d_out.data_ptr(), w + 8, h * (w + 8), w, h, n)
    safe_ctx.synchronize()
    got = d_out.cpu().numpy()
    assert (got[:, :, w:] == 7).all(), "wrote outside the frames' columns"
    for k in range(n):
        assert np.array_equal(got[k, :, :w], oracle.gpuorder_forward_y(frames[k], weights_blob)[0]), k
        assert np.array_equal(got[k, :, :w], safe_ctx.forward_y(frames[k])), k


# ---------------------------------------------------------------- 8. random weights

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_weights(safe_ctx, weights_blob, seed):
    """The generator and seeds of test_gpu_parity.py's test_random_weights_all_modes (weight fragments with other exponents e1, e2
    in the safe body): MODE_MFMA bitwise against the model and within that test's tolerance of the reference arithmetic,
    MODE_REFBYTES the reference's bytes, MODE_EXACT (which has one kernel form) the reference's bytes and floats."""
    rng = np.random.default_rng(seed)
    blob = weights_blob.copy()
    blob[64:5248] = rng.normal(0, 0.03, 5184).astype(np.float32)             # W1
    blob[0:64] = rng.normal(0, 1.0, 64).astype(np.float32)                    # b1
    blob[5280:7328] = rng.normal(0, 0.08, 2048).astype(np.float32)            # W2
    blob[5248:5280] = rng.normal(0, 1.0, 32).astype(np.float32)               # b2
    blob[7329:8129] = rng.normal(0, 0.02, 800).astype(np.float32)             # W3
    blob[7328] = np.float32(rng.normal(60, 10))                               # b3
    y = synth_luma(260, 75, frame=seed)
    r_out, r_pre = oracle.forward_y(y, blob)
    m_out, m_pre = oracle.gpuorder_forward_y(y, blob)
    scale = max(1.0, float(np.abs(r_pre).max()) / 255.0)
    try:
        safe_ctx.set_weights_blob(blob)
        pre = np.empty(y.shape, np.float32)
        out = safe_ctx.forward_y(y, preclamp=pre)
        assert np.array_equal(pre, m_pre) and np.array_equal(out, m_out)
        assert np.array_equal(safe_ctx.forward_y(y), m_out)
        assert np.abs(pre - r_pre).max() <= TOL_PRE_ABS * scale
        safe_ctx.set_mode(S.MODE_REFBYTES)
        reruns = safe_ctx.fixup_stats()["exact_reruns"]
        assert np.array_equal(safe_ctx.forward_y(y), r_out)
        assert safe_ctx.fixup_stats()["exact_reruns"] == reruns, "the re-run net fired"
        safe_ctx.set_mode(S.MODE_EXACT)
        e_pre = np.empty(y.shape, np.float32)
        e_out = safe_ctx.forward_y(y, preclamp=e_pre)
        assert np.array_equal(e_pre, r_pre) and np.array_equal(e_out, r_out)
    finally:
        safe_ctx.set_mode(S.MODE_MFMA)
        safe_ctx.set_weights_blob(weights_blob)


# ---------------------------------------------------------------- 9. 9-3-5 / 9-5-5 byte models: layer 3 through MODE_L3

@pytest.mark.parametrize("mode", [S.MODE_MFMA, S.MODE_BANDED16], ids=["MFMA", "BANDED16"])
@pytest.mark.parametrize("f2", [3, 5])
def test_byte_models_layer3(f2, mode):
    """1-channel, replicate padding: layers 1-2 on the banded path, layer 3 one run_strip(MODE_L3) per row band (srcnn_spatial.cpp)
    -- the safe MODE_L3 kernel with the band's map as its planes, with a pre-clamp plane (PRE) and without.  131 x 70 is one
    band; 3840 x 400 is two bands of 200 rows (band_max = 357 rows at this width for f2 = 5, 358 for f2 = 3).  Bytes and
    pre-clamp floats are bitwise those of a variant-0 context (layers 1-2 are the same kernels in both) and within
    test_gpu_spatial.py's tolerance of the float64 restatement; a row range that starts inside the first band and ends inside
    the second (srcnn_model_rows_dev) equals the whole plane's rows."""
    torch = _torch()
    model = random_model(f2, 17)
    with S.Context(0) as fast, S.Context(0) as safe:
        safe.set_kernel_variant(1)
        for c in (fast, safe):
            c.set_model(*model)
            c.set_mode(mode)
        assert (fast.kernel_variant(), safe.kernel_variant()) == (0, 1)
        for w, h in [(131, 70), (3840, 400)]:
            y = synth_luma(w, h, frame=f2)
            got = {}
            for name, c in (("fast", fast), ("safe", safe)):
                pre = np.empty(y.shape, np.float32)
                out = c.forward_y(y, preclamp=pre)                   # MODE_L3 with PRE
                got[name] = (out, pre, c.forward_y(y))               # MODE_L3 plain
            out, pre, plain = got["safe"]
            assert np.array_equal(plain, out)
            assert np.array_equal(out, got["fast"][0]) and np.array_equal(pre, got["fast"][1]) and np.array_equal(plain, got["fast"][2])
            if h == 70:
                assert band_seams(w, h, f2) == []
                check_spatial(out, pre, torch_forward(y, model))
                continue
            assert band_seams(w, h, f2) == [200]
            for r0, r1 in [(0, 24), (188, 212), (376, 400)]:        # the image's edges and the rows where the bands meet
                check_spatial(out[r0:r1], pre[r0:r1], torch_forward_rows(y, model, r0, r1))
            r0, r1 = 150, 330
            d_in = torch.from_numpy(y).cuda()
            d_out = torch.zeros((r1 - r0, w), dtype=torch.uint8, device="cuda")
            d_pre = torch.zeros((r1 - r0, w), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            safe.model_rows_dev(d_in.data_ptr(), w, 0, d_out.data_ptr(), w, r0, w, h, r0, r1, d_pre.data_ptr())
            safe.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), out[r0:r1]) and np.array_equal(d_pre.cpu().numpy(), pre[r0:r1])
        assert (fast.kernel_variant(), safe.kernel_variant()) == (0, 1)


# ---------------------------------------------------------------- 10. modes the variant does not reach, and state

@pytest.mark.parametrize("w,h", [(300, 70), (1920, 400)])
def test_split_f16_modes_have_one_kernel_form(safe_ctx, weights_blob, w, h):
    """SRCNN_MODE_SPLIT16 and SRCNN_MODE_REFBYTES16 launch srcnn_split16.hip, which exists once: pinned, they return the bytes of a
    variant-0 context, REFBYTES16 the reference's."""
    y, r_out, _ = plane(w, h, ITEM_FRAME if (w, h) in ITEM_PLANES else 5, weights_blob, reference=True)
    with S.Context(0) as fast:
        fast.set_weights_blob(weights_blob)
        assert fast.kernel_variant() == 0
        try:
            for mode in (S.MODE_SPLIT16, S.MODE_REFBYTES16):
                fast.set_mode(mode)
                safe_ctx.set_mode(mode)
                reruns = safe_ctx.fixup_stats()["exact_reruns"]
                got = safe_ctx.forward_y(y)
                assert np.array_equal(got, fast.forward_y(y)), mode
                if mode == S.MODE_REFBYTES16:
                    assert np.array_equal(got, r_out)
                    assert safe_ctx.fixup_stats()["exact_reruns"] == reruns, "the re-run net fired"
                else:
                    assert np.abs(got.astype(int) - r_out.astype(int)).max() <= 1
        finally:
            safe_ctx.set_mode(S.MODE_MFMA)


def test_the_pin_survives_every_setter(weights_blob):
    torch = _torch()
    y, m_out, _ = plane(300, 70, 5, weights_blob)
    stream = torch.cuda.Stream()
    with S.Context(0) as ctx:
        ctx.set_kernel_variant(1)
        steps = [
            ("set_weights_blob", lambda: ctx.set_weights_blob(weights_blob)),
            ("set_mode", lambda: (ctx.set_mode(S.MODE_REFBYTES), ctx.set_mode(S.MODE_SPLIT16), ctx.set_mode(S.MODE_EXACT), ctx.set_mode(S.MODE_MFMA))),
            ("set_model", lambda: ctx.set_model(*random_model(3, 1))),
            ("set_padding", lambda: (ctx.set_padding("zero"), ctx.set_padding("replicate"))),
            ("set_weights_blob again", lambda: ctx.set_weights_blob(weights_blob)),
            ("set_seam_deferral", lambda: (ctx.set_seam_deferral(True), ctx.set_seam_deferral(False))),
            ("set_stream", lambda: (ctx.set_stream(stream.cuda_stream), ctx.set_stream(0))),
        ]
        for name, step in steps:
            step()
            assert ctx.kernel_variant() == 1, f"{name} reset the kernel variant"
        assert np.array_equal(ctx.forward_y(y), m_out)
        assert ctx.kernel_variant() == 1


def test_two_contexts_one_per_variant_on_one_stream(weights_blob):
    """The per-device probe verdict and the item-table caches are shared state; the variant is the context's own.  A fast and a
    pinned context on the SAME torch stream alternate launches of 1920 x 400 (work items with seams): every output is the
    model's, neither context changes the other's variant, and a context created after the pin is variant 0."""
    torch = _torch()
    w, h = ITEM_PLANES[0]
    y, m_out, _ = plane(w, h, ITEM_FRAME, weights_blob)
    stream = torch.cuda.Stream()
    with S.Context(0) as fast, S.Context(0) as safe:
        safe.set_kernel_variant(1)
        for c in (fast, safe):
            c.set_weights_blob(weights_blob)
            c.set_stream(stream.cuda_stream)
        with S.Context(0) as later:
            assert later.kernel_variant() == 0, "pinning one context pinned the device"
        d_in = torch.from_numpy(y).cuda()
        outs = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(6)]
        torch.cuda.synchronize()
        order = [fast, safe, fast, safe, safe, fast]
        for c, o in zip(order, outs):
            c.forward_y_dev(d_in.data_ptr(), w, 0, o.data_ptr(), w, 0, w, h, 1)
            assert (fast.kernel_variant(), safe.kernel_variant()) == (0, 1)
        stream.synchronize()
        for k, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy(), m_out), f"launch {k} ({'safe' if order[k] is safe else 'fast'})"
        fast.set_kernel_variant(0)                        # asking for the probe's verdict again changes nothing for the other
        assert (fast.kernel_variant(), safe.kernel_variant()) == (0, 1)
        for c in (fast, safe):
            c.set_stream(0)


def test_deferral_asked_for_is_not_used(weights_blob):
    """Seam deferral under variant 1: three device launches queued back to back on the caller's stream, no srcnn_flush and no
    other call on the context, then a synchronize of the STREAM alone -- the safe form queues every launch's seam work with the
    launch, so all three outputs are complete and the model's."""
    torch = _torch()
    w, h = ITEM_PLANES[0]
    y, m_out, _ = plane(w, h, ITEM_FRAME, weights_blob)
    stream = torch.cuda.Stream()
    with S.Context(0) as ctx:
        ctx.set_weights_blob(weights_blob)
        ctx.set_kernel_variant(1)
        ctx.set_stream(stream.cuda_stream)
        ctx.set_seam_deferral(True)
        d_in = torch.from_numpy(y).cuda()
        outs = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        for o in outs:
            ctx.forward_y_dev(d_in.data_ptr(), w, 0, o.data_ptr(), w, 0, w, h, 1)
        stream.synchronize()
        got = [o.cpu().numpy() for o in outs]
        assert ctx.kernel_variant() == 1
        for k in range(3):
            assert np.array_equal(got[k], m_out), f"launch {k} is incomplete or wrong"
        ctx.set_seam_deferral(False)
        ctx.set_stream(0)


def test_lanes_of_two_pinned_contexts(weights_blob):
    """srcnn_forward_y_lanes_dev switches deferral on in its lanes' contexts for the call: two pinned contexts, four 576 x 576
    planes, each the model's after a synchronize per context."""
    torch = _torch()
    w = h = 576
    n = 4
    frames = synth_batch(w, h, n, first_frame=60)
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.zeros_like(d_in)
    ctxs = [S.Context(0) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    try:
        for c, st in zip(ctxs, streams):
            c.set_weights_blob(weights_blob)
            c.set_kernel_variant(1)
            c.set_stream(st.cuda_stream)
        torch.cuda.synchronize()
        S.forward_y_lanes_dev(ctxs, [d_in[k].data_ptr() for k in range(n)], w, [d_out[k].data_ptr() for k in range(n)], w, w, h)
        for c in ctxs:
            c.synchronize()
            assert c.kernel_variant() == 1
        got = d_out.cpu().numpy()
        for k in range(n):
            assert np.array_equal(got[k], oracle.gpuorder_forward_y(frames[k], weights_blob)[0]), k
    finally:
        for c in ctxs:
            c.close()
