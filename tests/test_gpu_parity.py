"""GPU parity tests: the HIP path, called THROUGH THE C ABI, against the oracle.

Two kinds of comparison:

* vs ``oracle.*``          -- the reference's arithmetic (strict multiply-then-add,
                              src/srcnn.cpp:92-325).  This is the parity claim.
                              SRCNN_MODE_EXACT and the per-filter entry points
                              (Convolution99 / Convolution11) must be BIT-EXACT;
                              the MFMA path must be within the float32 tolerance
                              below.
* vs ``oracle.gpuorder_*`` -- a CPU model of the MFMA kernels' summation order
                              (FMA chains); must be BITWISE equal, so a layout or
                              indexing bug can never hide inside the tolerance.

Float32 tolerance of the MFMA path vs the reference arithmetic (north_star:
"within a stated float32 tolerance"):
    32-channel map after layer 2 : |d| <= 1e-3 * max(1, |ref|)
    pre-clamp f32 output         : |d| <= 5e-3   (0..255 scale)
    u8 output                    : |d| <= 1 LSB everywhere; a pixel may differ ONLY where the
                                   reference's pre-truncation value lies within 5e-3 of an
                                   integer (the store truncates, src/srcnn.cpp:238-240);
                                   on planes >= 1e5 pixels mismatches <= 1e-3 of pixels
"""
import numpy as np
import pytest

import oracle
import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma, synth_batch

pytestmark = pytest.mark.gpu

TOL_MAP_REL = 1e-3
TOL_PRE_ABS = 5e-3
TOL_U8_FRAC = 1e-3

EDGE_SIZES = [(1, 1), (3, 3), (9, 5), (5, 9), (17, 4), (2, 40), (40, 2), (31, 7), (33, 9)]
TILE_SIZES = [(123, 11), (124, 13), (125, 9), (127, 6), (128, 20), (129, 10), (248, 7), (249, 8),
              (300, 70), (97, 61)]


def planes32(h, w, stride=None):
    stride = stride or w
    buf = np.zeros((32, h, stride), np.float32)
    return buf, [buf[k, :, :w] for k in range(32)]


def check_u8(got, ref, ref_pre=None):
    d = np.abs(got.astype(int) - ref.astype(int))
    assert d.max() <= 1, f"u8 differs by {d.max()} LSB"
    if ref_pre is not None and d.any():
        near = np.abs(ref_pre - np.rint(ref_pre))[d != 0]
        assert near.max() <= TOL_PRE_ABS, "u8 mismatch away from a truncation boundary"
    if d.size >= 100000 or ref_pre is None:
        assert (d != 0).sum() <= max(2, TOL_U8_FRAC * d.size), f"{(d != 0).sum()} of {d.size} pixels differ"


# ---------------------------------------------------------------- Convolution99 / 11 (bit-exact)

@pytest.mark.parametrize("w,h", EDGE_SIZES + [(97, 61), (200, 33)])
def test_conv99_bit_exact(gpu_ctx, weights_blob, w, h):
    w1, b1, *_ = S.split_weights(weights_blob)
    y = synth_luma(w, h, frame=2)
    for k in (0, 8, 63):
        dst = np.full((h, w), -7.0, np.float32)
        gpu_ctx.conv99(y, dst, w1[k], b1[k])
        assert np.array_equal(dst, oracle.conv99(y, w1[k], b1[k]))


@pytest.mark.parametrize("w,h", [(1, 1), (9, 5), (70, 33), (129, 17)])
def test_conv11_bit_exact(gpu_ctx, weights_blob, w, h):
    w1, b1, w2, b2, *_ = S.split_weights(weights_blob)
    rng = np.random.default_rng(w * 1000 + h)
    src = (rng.random((64, h, w), dtype=np.float32) * 300).astype(np.float32)
    src[rng.random((64, h, w)) < 0.4] = 0
    for k in (0, 31):
        dst = np.empty((h, w), np.float32)
        gpu_ctx.conv11([src[i] for i in range(64)], dst, w2[k], b2[k])
        assert np.array_equal(dst, oracle.conv11(src, w2[k], b2[k]))


def test_unfused_surface_equals_fused_oracle(gpu_ctx, weights_blob):
    """64 x Convolution99 then 32 x Convolution11 on the GPU == the reference's
    fused Convolution99x11, bit for bit."""
    w1, b1, w2, b2, *_ = S.split_weights(weights_blob)
    y = synth_luma(45, 23, frame=5)
    l1 = np.empty((64, 23, 45), np.float32)
    for k in range(64):
        gpu_ctx.conv99(y, l1[k], w1[k], b1[k])
    l2 = np.empty((32, 23, 45), np.float32)
    for k in range(32):
        gpu_ctx.conv11([l1[i] for i in range(64)], l2[k], w2[k], b2[k])
    assert np.array_equal(l2, oracle.conv99x11(y, w1, b1, w2, b2))


# ---------------------------------------------------------------- Convolution99x11 (MFMA)

@pytest.mark.parametrize("w,h", EDGE_SIZES + TILE_SIZES)
def test_conv99x11_mfma(gpu_ctx, weights_blob, w, h):
    w1, b1, w2, b2, *_ = S.split_weights(weights_blob)
    y = synth_luma(w, h, frame=1)
    buf, dst = planes32(h, w)
    buf[:] = -1.0
    gpu_ctx.conv99x11(y, dst, w1, b1, w2, b2)
    model = oracle.gpuorder_conv99x11(y, w1, b1, w2, b2)
    assert np.array_equal(buf, model), "MFMA layer 1-2 differs from its FMA-order model"
    ref = oracle.conv99x11(y, w1, b1, w2, b2)
    assert (np.abs(buf - ref) <= TOL_MAP_REL * np.maximum(1.0, np.abs(ref))).all()


def test_conv99x11_strided_planes(gpu_ctx, weights_blob):
    w1, b1, w2, b2, *_ = S.split_weights(weights_blob)
    ybuf = np.zeros((30, 80), np.uint8)
    ybuf[:, :71] = synth_luma(71, 30)
    y = ybuf[:, :71]
    buf, dst = planes32(30, 71, stride=96)
    buf[:] = np.float32(-5)
    gpu_ctx.conv99x11(y, dst, w1, b1, w2, b2)
    assert np.array_equal(buf[:, :, :71], oracle.gpuorder_conv99x11(np.ascontiguousarray(y), w1, b1, w2, b2))
    assert (buf[:, :, 71:] == -5).all(), "wrote outside the plane's columns"


# ---------------------------------------------------------------- Convolution55 (MFMA)

@pytest.mark.parametrize("w,h", EDGE_SIZES + TILE_SIZES)
def test_conv55_mfma(gpu_ctx, weights_blob, w, h):
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    feat = oracle.conv99x11(synth_luma(w, h, frame=4), w1, b1, w2, b2)
    dst = np.full((h, w), 77, np.uint8)
    gpu_ctx.conv55([feat[k] for k in range(32)], dst, w3, b3)
    model, _ = oracle.gpuorder_conv55(feat, w3, b3)
    assert np.array_equal(dst, model), "MFMA layer 3 differs from its FMA-order model"
    ref, ref_pre = oracle.conv55(feat, w3, b3)
    check_u8(dst, ref, ref_pre)


# ---------------------------------------------------------------- whole path, fused kernel

@pytest.mark.parametrize("w,h", EDGE_SIZES + TILE_SIZES)
def test_forward_fused(gpu_ctx, weights_blob, w, h):
    y = synth_luma(w, h)
    pre = np.empty((h, w), np.float32)
    out = gpu_ctx.forward_y(y, preclamp=pre)
    m_out, m_pre = oracle.gpuorder_forward_y(y, weights_blob)
    assert np.array_equal(pre, m_pre), "fused kernel differs from its FMA-order model (pre-clamp)"
    assert np.array_equal(out, m_out)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    assert np.abs(pre - r_pre).max() <= TOL_PRE_ABS
    check_u8(out, r_out, r_pre)


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_forward_constant_images(gpu_ctx, weights_blob, value):
    y = np.full((37, 150), value, np.uint8)
    out = gpu_ctx.forward_y(y)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    check_u8(out, r_out, r_pre)
    assert (out == out[0, 0]).all()


def test_forward_saturating_input(gpu_ctx, weights_blob):
    """i.i.d. bytes drive the output into the 0/255 clamp (src/srcnn.cpp:238)."""
    y = np.random.default_rng(7).integers(0, 256, (64, 140), dtype=np.uint8)
    out = gpu_ctx.forward_y(y)
    m_out, _ = oracle.gpuorder_forward_y(y, weights_blob)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    assert np.array_equal(out, m_out)
    assert ((r_out == 0) | (r_out == 255)).mean() > 0.2
    check_u8(out, r_out, r_pre)


def test_forward_strided_host_planes(gpu_ctx, weights_blob):
    ybuf = np.zeros((41, 160), np.uint8)
    ybuf[:, 3:133] = synth_luma(130, 41)
    y = ybuf[:, 3:133]
    obuf = np.full((41, 200), 9, np.uint8)
    gpu_ctx.forward_y(y, dst=obuf[:, :130])
    m_out, _ = oracle.gpuorder_forward_y(np.ascontiguousarray(y), weights_blob)
    assert np.array_equal(obuf[:, :130], m_out)
    assert (obuf[:, 130:] == 9).all()


def test_butterfly_fixture(gpu_ctx, weights_blob):
    """configs[0] input (butterfly.png x1.5) through the GPU path: equals the
    oracle within tolerance and lands on the reference's own output picture."""
    from pathlib import Path
    gold = Path(__file__).resolve().parent / "golden"
    y_in = np.fromfile(gold / "butterfly_y_in_576.u8", np.uint8).reshape(576, 576)
    y_ref = np.fromfile(gold / "butterfly_y_ref_576.u8", np.uint8).reshape(576, 576)
    out = gpu_ctx.forward_y(y_in)
    r_out, r_pre = oracle.forward_y(y_in, weights_blob)
    check_u8(out, r_out, r_pre)
    d = out.astype(np.float64) - y_ref
    assert 10 * np.log10(255.0 ** 2 / np.mean(d * d)) >= 50.0


# ---------------------------------------------------------------- SRCNN_MODE_EXACT (bit-exact)

@pytest.mark.parametrize("w,h", [(1, 1), (9, 5), (5, 9), (97, 61), (130, 20)])
def test_exact_mode_bit_exact(gpu_ctx, weights_blob, w, h):
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    y = synth_luma(w, h, frame=6)
    gpu_ctx.set_mode(S.MODE_EXACT)
    try:
        pre = np.empty((h, w), np.float32)
        out = gpu_ctx.forward_y(y, preclamp=pre)
        buf, dst = planes32(h, w)
        gpu_ctx.conv99x11(y, dst, w1, b1, w2, b2)
        o55 = np.empty((h, w), np.uint8)
        gpu_ctx.conv55([buf[k] for k in range(32)], o55, w3, b3)
    finally:
        gpu_ctx.set_mode(S.MODE_MFMA)
        gpu_ctx.set_weights_blob(weights_blob)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    assert np.array_equal(buf, oracle.conv99x11(y, w1, b1, w2, b2))
    assert np.array_equal(pre, r_pre)
    assert np.array_equal(out, r_out) and np.array_equal(o55, r_out)


# ---------------------------------------------------------------- device-resident API, batches, stripes

def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_device_batch_and_unfused_agree(gpu_ctx, weights_blob):
    """configs[2] shape in miniature: a batch of frames through the fused kernel
    and through the materialising (layer-1/2 kernel + layer-3 kernel) path give
    identical bytes, and each frame equals the single-frame result."""
    torch = _torch()
    n, h, w = 5, 45, 200
    frames = synth_batch(w, h, n)
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.zeros_like(d_in)
    d_out2 = torch.zeros_like(d_in)
    d_work = torch.empty((n, 32, h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.forward_y_dev(d_in.data_ptr(), w, h * w, d_out.data_ptr(), w, h * w, w, h, n)
    gpu_ctx.forward_y_unfused_dev(d_in.data_ptr(), w, h * w, d_out2.data_ptr(), w, h * w, w, h, n,
                                  d_work.data_ptr())
    gpu_ctx.synchronize()
    a, b = d_out.cpu().numpy(), d_out2.cpu().numpy()
    assert np.array_equal(a, b)
    for k in range(n):
        m_out, _ = oracle.gpuorder_forward_y(frames[k], weights_blob)
        assert np.array_equal(a[k], m_out)


def test_small_batch_repeats_the_item_plan_per_frame(gpu_ctx, weights_blob):
    """A batch of fewer than 32 frames runs the single-plane work items (row and column seams, no halo rows) frame after
    frame in ONE launch; every frame must equal the plane computed alone, with padded strides and frame pitches."""
    torch = _torch()
    n, h, w = 3, 1080, 1920
    assert gpu_ctx.query_plan(w, h, n)["workgroups"] == n * gpu_ctx.query_plan(w, h, 1)["workgroups"]
    frames = synth_batch(w, h, n, first_frame=20)
    pitch = (h + 3) * (w + 64)
    d_in = torch.zeros((n, pitch), dtype=torch.uint8, device="cuda")
    d_in[:, : h * (w + 64)].view(n, h, w + 64)[:, :, :w] = torch.from_numpy(frames).cuda()
    d_out = torch.full((n, pitch), 7, dtype=torch.uint8, device="cuda")
    d_pre = torch.zeros((n, pitch), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.forward_y_dev(d_in.data_ptr(), w + 64, pitch, d_out.data_ptr(), w + 64, pitch, w, h, n, d_pre.data_ptr())
    gpu_ctx.synchronize()
    got = d_out[:, : h * (w + 64)].view(n, h, w + 64).cpu().numpy()
    pre = d_pre[:, : h * (w + 64)].view(n, h, w + 64).cpu().numpy()
    assert (got[:, :, w:] == 7).all(), "wrote outside the frames' columns"
    for k in range(n):
        alone_pre = np.empty((h, w), np.float32)
        alone = gpu_ctx.forward_y(frames[k], preclamp=alone_pre)
        assert np.array_equal(got[k, :, :w], alone) and np.array_equal(pre[k, :, :w], alone_pre)
    m_out, _ = oracle.gpuorder_forward_y(frames[1], weights_blob)
    assert np.array_equal(got[1, :, :w], m_out)


@pytest.mark.parametrize("n_stripes", [2, 3, 8])
def test_row_stripes_equal_whole_image(gpu_ctx, weights_blob, n_stripes):
    """configs[3] in miniature: row stripes with a 6-row input halo stitch to the
    whole-image result bit for bit (image edges replicate, stripe edges do not)."""
    torch = _torch()
    h, w = 90, 260
    y = synth_luma(w, h, frame=9)
    whole = gpu_ctx.forward_y(y)
    out = np.zeros_like(y)
    bounds = np.linspace(0, h, n_stripes + 1).astype(int)
    for s in range(n_stripes):
        r0, r1 = int(bounds[s]), int(bounds[s + 1])
        s0, s1 = max(0, r0 - 6), min(h, r1 + 6)
        d_in = torch.from_numpy(np.ascontiguousarray(y[s0:s1])).cuda()
        d_out = torch.zeros((r1 - r0, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.forward_y_rows_dev(d_in.data_ptr(), w, s0, d_out.data_ptr(), w, r0, w, h, r0, r1)
        gpu_ctx.synchronize()
        out[r0:r1] = d_out.cpu().numpy()
    assert np.array_equal(out, whole)


@pytest.mark.parametrize("mode", [S.MODE_MFMA, S.MODE_REFBYTES])
@pytest.mark.parametrize("w,h,n_stripes", [(260, 90, 2), (260, 90, 3), (260, 97, 8), (3840, 601, 3), (1000, 340, 4)])
def test_row_stripes_with_halo_rows_in_their_own_buffers(weights_blob, mode, w, h, n_stripes):
    """srcnn_forward_y_rows_halo_dev: a rank's rows where they lie (an exactly sized allocation), the 6 rows of each
    neighbour in small buffers of their own with another row stride -- ONE launch per stripe, and the stitched plane is
    the whole-image result bit for bit (the model's bytes in the MFMA mode, the reference's in SRCNN_MODE_REFBYTES).
    3840x601 runs as work items with seams and the FAST row body, the small planes on the regular grid."""
    torch = _torch()
    y = synth_luma(w, h, frame=13)
    want = oracle.gpuorder_forward_y(y, weights_blob)[0] if mode == S.MODE_MFMA else oracle.forward_y(y, weights_blob)[0]
    with S.Context(0) as ctx:
        ctx.set_weights_blob(weights_blob)
        ctx.set_mode(mode)
        out = np.zeros_like(y)
        for k in range(n_stripes):
            r0, r1 = S.stripe_rows(h, n_stripes, k)
            d_own = torch.from_numpy(np.ascontiguousarray(y[r0:r1])).cuda()
            hs = w + 20                                             # the halo buffers' own row stride
            top = bot = None
            if k > 0:
                top = torch.full((6, hs), 77, dtype=torch.uint8, device="cuda")
                top[:, :w] = torch.from_numpy(np.ascontiguousarray(y[r0 - 6:r0])).cuda()
            if k < n_stripes - 1:
                bot = torch.full((6, hs), 77, dtype=torch.uint8, device="cuda")
                bot[:, :w] = torch.from_numpy(np.ascontiguousarray(y[r1:r1 + 6])).cuda()
            d_out = torch.zeros((r1 - r0, w), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, top.data_ptr() if top is not None else 0,
                                        bot.data_ptr() if bot is not None else 0, hs, d_out.data_ptr(), w, r0, w, h, r0, r1)
            ctx.synchronize()
            out[r0:r1] = d_out.cpu().numpy()
        assert np.array_equal(out, want)
        # a sub-range of a stripe that needs only ONE of the halos, and one that needs none (both pointers may then be null)
        r0, r1 = S.stripe_rows(h, n_stripes, 1)
        d_own = torch.from_numpy(np.ascontiguousarray(y[r0:r1])).cuda()
        top = torch.from_numpy(np.ascontiguousarray(y[r0 - 6:r0])).cuda()
        d_out = torch.zeros((r1 - r0, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if r1 - r0 >= 14:
            ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, top.data_ptr(), 0, w, d_out.data_ptr(), w, r0, w, h, r0, r1 - 6)
            ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, 0, 0, w, d_out.data_ptr(), w, r0, w, h, r0 + 6, r1 - 6)
            ctx.synchronize()
            assert np.array_equal(d_out.cpu().numpy()[:r1 - r0 - 6], want[r0:r1 - 6])
        # rows the buffers do not cover are refused, not read
        with pytest.raises(S.SrcnnError) as e:
            ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, 0, 0, w, d_out.data_ptr(), w, r0, w, h, r0, r1 - 6)
        assert e.value.code == S.ERR_INVALID
        if n_stripes > 2:
            with pytest.raises(S.SrcnnError):
                ctx.forward_y_rows_halo_dev(d_own.data_ptr(), w, r0, r1 - r0, top.data_ptr(), 0, w, d_out.data_ptr(), w, r0, w, h, r0, r1)


@pytest.mark.parametrize("w,h", [(300, 97), (3840, 601)])
def test_row_ranges_of_every_alignment(gpu_ctx, weights_blob, w, h):
    """The steady-state rows of a work item run through a row body that is unrolled over four rows and finishes two
    output rows at once (csrc/srcnn_mfma.hip, FAST body); the rows before the first and behind the last multiple of
    four, the image's first and last rows and the rows next to a seam or a stripe edge go through the general body.
    Every alignment of a row range against that period -- first row 0..9, last row H-9..H, short and tall ranges, padded
    output rows -- must give the bytes of the whole-image model.  300x97 runs on the regular grid (short segments,
    general body only), 3840x601 as work items of ~35 rows with seams (FAST body in the middle of every item)."""
    torch = _torch()
    y = synth_luma(w, h, frame=21)
    model, _ = oracle.gpuorder_forward_y(y, weights_blob)
    assert np.array_equal(gpu_ctx.forward_y(y), model)
    d_in = torch.from_numpy(y).cuda()
    ranges = [(r0, r1) for r0 in range(0, 10) for r1 in (h, h - 1, h - 2, h - 3, h - 5, h - 9)]
    ranges += [(r0, r0 + n) for r0 in (0, 3, 14, 41) for n in (1, 2, 5, 11, 12, 13, 19, 24, 31)]
    if h > 400:
        ranges += [(r0, r0 + n) for r0 in (7, 100, 233) for n in (200, 257, 300, 366)]
    for r0, r1 in ranges:
        d_out = torch.full((r1 - r0, w + 12), 5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.forward_y_rows_dev(d_in.data_ptr(), w, 0, d_out.data_ptr(), w + 12, r0, w, h, r0, r1)
        gpu_ctx.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:, :w], model[r0:r1]), (r0, r1)
        assert (got[:, w:] == 5).all(), (r0, r1)    # nothing written beyond the row


@pytest.mark.parametrize("w,h", [(3840, 2160), (1920, 1080), (2000, 1203), (992, 1700), (7680, 4320), (125, 6400)])
def test_single_plane_work_items_equal_batch_grid(gpu_ctx, weights_blob, w, h):
    """Launch-geometry independence at full sizes: a plane launched alone is cut into
    unequal per-block work items sized for the wave slot they land in
    (csrc/srcnn_plan.cpp plan_items); inside a batch the same plane runs on the regular
    strip x segment grid.  Both must give the same bytes -- any gap or overlap in the item
    table shows up here.  A row stripe of the plane (row_begin != 0) is checked too."""
    torch = _torch()
    y = synth_luma(w, h, frame=3)
    d_in = torch.from_numpy(np.stack([y, y])).cuda()
    d_batch = torch.zeros_like(d_in)
    d_one = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.forward_y_dev(d_in.data_ptr(), w, h * w, d_batch.data_ptr(), w, h * w, w, h, 2)
    gpu_ctx.forward_y_dev(d_in.data_ptr(), w, h * w, d_one.data_ptr(), w, h * w, w, h, 1)
    gpu_ctx.synchronize()
    batch = d_batch.cpu().numpy()
    one = d_one.cpu().numpy()
    assert np.array_equal(batch[0], batch[1])
    assert np.array_equal(one, batch[0])
    plan1, plan2 = gpu_ctx.query_plan(w, h, 1), gpu_ctx.query_plan(w, h, 2)
    assert plan1["workgroups"] >= 1 and plan2["workgroups"] >= 2
    r0, r1 = h // 3 + 1, h - h // 5
    d_stripe = torch.full((r1 - r0, w), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.forward_y_rows_dev(d_in.data_ptr(), w, 0, d_stripe.data_ptr(), w, r0, w, h, r0, r1)
    gpu_ctx.synchronize()
    assert np.array_equal(d_stripe.cpu().numpy(), one[r0:r1])


def test_full_size_4k_frame(gpu_ctx, weights_blob):
    """configs[1] at full size (3840x2160).  The whole frame is checked bitwise
    against the FMA-order model; parity with the reference arithmetic is checked
    on the whole frame too (oracle, all host cores)."""
    w, h = 3840, 2160
    y = synth_luma(w, h)
    pre = np.empty((h, w), np.float32)
    out = gpu_ctx.forward_y(y, preclamp=pre)
    # without the optional pre-clamp plane the host entry point pipelines the plane through in four row bands
    # (uploads, launches and downloads of neighbouring bands overlap): same bytes
    assert np.array_equal(gpu_ctx.forward_y(y), out)
    padded = np.zeros((h, w + 64), np.uint8)
    padded[:, :w] = y
    dst = np.zeros((h, w + 32), np.uint8)
    assert np.array_equal(gpu_ctx.forward_y(padded[:, :w], dst=dst[:, :w]), out)      # padded row strides, both sides
    # size-independent property: 13x13 locality -- crops reproduce the frame
    for (r0, c0) in [(0, 0), (1000, 2000), (h - 80, w - 200), (0, w - 150), (h - 64, 0)]:
        r1, c1 = min(h, r0 + 80), min(w, c0 + 200)
        crop = np.ascontiguousarray(y[r0:r1, c0:c1])
        c_out = gpu_ctx.forward_y(crop)
        ir0, ic0 = (0 if r0 == 0 else 6), (0 if c0 == 0 else 6)
        ir1, ic1 = (r1 - r0 if r1 == h else r1 - r0 - 6), (c1 - c0 if c1 == w else c1 - c0 - 6)
        assert np.array_equal(c_out[ir0:ir1, ic0:ic1], out[r0 + ir0:r0 + ir1, c0 + ic0:c0 + ic1])
    # committed checksums of this frame, computed in the build container (tests/golden/make_4k_checksums.py)
    import hashlib, json
    from pathlib import Path
    pins = json.loads((Path(__file__).resolve().parent / "golden" / "synthetic_4k_checksums.json").read_text())
    assert hashlib.sha256(y.tobytes()).hexdigest() == pins["input_sha256"]
    assert hashlib.sha256(out.tobytes()).hexdigest() == pins["gpuorder_sha256"]
    m_out, m_pre = oracle.gpuorder_forward_y(y, weights_blob)
    assert np.array_equal(pre, m_pre)
    assert np.array_equal(out, m_out)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    assert hashlib.sha256(r_out.tobytes()).hexdigest() == pins["oracle_sha256"]
    assert int((out != r_out).sum()) == pins["u8_mismatches_between_them"]
    # SRCNN_MODE_EXACT reproduces the reference arithmetic bit for bit at full size
    gpu_ctx.set_mode(S.MODE_EXACT)
    try:
        e_pre = np.empty((h, w), np.float32)
        e_out = gpu_ctx.forward_y(y, preclamp=e_pre)
    finally:
        gpu_ctx.set_mode(S.MODE_MFMA)
    assert hashlib.sha256(e_out.tobytes()).hexdigest() == pins["oracle_sha256"]
    assert np.array_equal(e_pre, r_pre)
    assert np.abs(pre - r_pre).max() <= TOL_PRE_ABS
    check_u8(out, r_out, r_pre)


def test_in_place_calls_are_rejected(gpu_ctx):
    """Every output pixel reads a 13 x 13 input window that other workgroups may already have overwritten: src and dst of
    the device entry point must not overlap (the reference writes a separate Mat too, src/srcnn.cpp:625-626)."""
    torch = _torch()
    w, h = 256, 64
    buf = torch.zeros((2 * h, w), dtype=torch.uint8, device="cuda")
    with pytest.raises(S.SrcnnError):
        gpu_ctx.forward_y_dev(buf.data_ptr(), w, h * w, buf.data_ptr(), w, h * w, w, h, 1)
    with pytest.raises(S.SrcnnError):                       # partial overlap: dst starts inside src
        gpu_ctx.forward_y_dev(buf.data_ptr(), w, h * w, buf.data_ptr() + 10 * w, w, h * w, w, h, 1)
    gpu_ctx.forward_y_dev(buf.data_ptr(), w, h * w, buf.data_ptr() + h * w, w, h * w, w, h, 1)     # adjacent halves: fine
    gpu_ctx.synchronize()
    # the stripe entry point with separate halo buffers: the output rows may overlap neither the stripe nor a halo buffer
    own, halo, out = buf[:32], torch.zeros((6, w), dtype=torch.uint8, device="cuda"), torch.zeros((32, w), dtype=torch.uint8, device="cuda")
    args = lambda dst, top, bot: (own.data_ptr(), w, 16, 32, top, bot, w, dst, w, 16, w, h, 16, 48)
    for dst, top, bot in ((own.data_ptr(), halo.data_ptr(), halo.data_ptr()), (out.data_ptr(), out.data_ptr(), halo.data_ptr()),
                          (out.data_ptr(), halo.data_ptr(), out.data_ptr() + 20 * w)):
        with pytest.raises(S.SrcnnError):
            gpu_ctx.forward_y_rows_halo_dev(*args(dst, top, bot))
    gpu_ctx.forward_y_rows_halo_dev(*args(out.data_ptr(), halo.data_ptr(), halo.data_ptr()))
    gpu_ctx.synchronize()


def test_error_paths(gpu_ctx):
    with pytest.raises(S.SrcnnError):
        gpu_ctx.forward_y_dev(0, 10, 100, 0, 10, 100, 10, 10, 1)
    ctx2 = S.Context(0)
    with pytest.raises(S.SrcnnError) as e:
        ctx2.forward_y(np.zeros((4, 4), np.uint8))
    assert e.value.code == -5            # SRCNN_ERR_STATE: no weights yet
    with pytest.raises(S.SrcnnError):
        S.Context(99)
    ctx2.close()


def test_cpp_host_through_reference_call_surface(tmp_path, weights_blob):
    """A plain C++ host (tools/host_demo.cpp: no OpenCV, no HIP headers) calls
    Convolution99x11 + Convolution55 with the reference's argument lists
    (src/srcnn.cpp:609,627) and the fused ForwardY; both must give the plane the
    FMA-order model predicts and sit within tolerance of the oracle."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "host_demo"
    subprocess.run(["g++", "-std=c++17", f"-I{root / 'include'}", str(root / "tools" / "host_demo.cpp"),
                    f"-L{root / 'srcnn_cpp_amd'}", "-lsrcnn_amd", f"-Wl,-rpath,{root / 'srcnn_cpp_amd'}",
                    "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    w, h = 200, 45
    out_file = tmp_path / "out.u8"
    res = subprocess.run([str(exe), str(S._WEIGHTS_PATH), str(w), str(h), str(out_file)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(out_file, np.uint8).reshape(h, w)
    y = synth_luma(w, h)
    m_out, _ = oracle.gpuorder_forward_y(y, weights_blob)
    r_out, r_pre = oracle.forward_y(y, weights_blob)
    assert np.array_equal(got, m_out)
    check_u8(got, r_out, r_pre)


def test_fused_kernel_is_deterministic_under_load(gpu_ctx, weights_blob):
    """Race screen: the fused kernel hands data between waves through LDS (T tiles,
    accumulator ring, Y ring) with one barrier per row.  Back-to-back launches on a
    busy GPU, several plane shapes, every byte compared: all runs must be identical
    (and equal to the model)."""
    import torch
    for (w, h, n) in [(3840, 2160, 12), (1000, 333, 40), (130, 700, 40)]:
        y = synth_luma(w, h, frame=11)
        d_in = torch.from_numpy(y).cuda()
        outs = [torch.empty_like(d_in) for _ in range(n)]
        torch.cuda.synchronize()
        for o in outs:                                   # queued back to back, no host sync in between
            gpu_ctx.forward_y_dev(d_in.data_ptr(), w, w * h, o.data_ptr(), w, w * h, w, h, 1)
        gpu_ctx.synchronize()
        first = outs[0].cpu().numpy()
        for o in outs[1:]:
            assert torch.equal(o, outs[0])
        if w * h < 500000:
            m_out, _ = oracle.gpuorder_forward_y(y, weights_blob)
            assert np.array_equal(first, m_out)


def test_host_frame_stream(gpu_ctx, weights_blob):
    """configs[4] shape in miniature through srcnn_forward_y_frames: a stream of host frames
    with overlapped transfers gives the same bytes as frame-by-frame calls."""
    frames = synth_batch(300, 77, 7, first_frame=20)
    out = gpu_ctx.forward_y_frames(frames)
    for k in range(7):
        assert np.array_equal(out[k], gpu_ctx.forward_y(frames[k]))
    m_out, _ = oracle.gpuorder_forward_y(frames[3], weights_blob)
    assert np.array_equal(out[3], m_out)
    one = gpu_ctx.forward_y_frames(frames[:1])
    assert np.array_equal(one[0], out[0])


def test_random_shapes_and_strides(gpu_ctx, weights_blob):
    """Randomised sweep: plane sizes 1..400 (biased to strip / unit boundaries), padded row
    strides on both sides, all three MFMA entry points -- every result bitwise equal to the
    FMA-order model and within tolerance of the reference arithmetic."""
    rng = np.random.default_rng(20261002)
    w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
    special = [1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 123, 124, 125, 127, 128, 129, 247, 248, 249, 372]
    for it in range(28):
        w = int(rng.choice(special)) if rng.random() < 0.6 else int(rng.integers(1, 400))
        h = int(rng.choice(special[:17])) if rng.random() < 0.5 else int(rng.integers(1, 120))
        pad_in, pad_out = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        ybuf = np.zeros((h, w + pad_in), np.uint8)
        ybuf[:, :w] = synth_luma(w, h, frame=it) if it % 4 else rng.integers(0, 256, (h, w), dtype=np.uint8)
        y = ybuf[:, :w]
        yc = np.ascontiguousarray(y)
        obuf = np.full((h, w + pad_out), 3, np.uint8)
        gpu_ctx.forward_y(y, dst=obuf[:, :w])
        m_out, _ = oracle.gpuorder_forward_y(yc, weights_blob)
        r_out, r_pre = oracle.forward_y(yc, weights_blob)
        assert np.array_equal(obuf[:, :w], m_out), (w, h, pad_in, pad_out)
        assert (obuf[:, w:] == 3).all()
        check_u8(obuf[:, :w], r_out, r_pre)
        if it % 3 == 0:      # the two-kernel surface on the same plane
            buf, dst = planes32(h, w, stride=w + pad_out)
            gpu_ctx.conv99x11(y, dst, w1, b1, w2, b2)
            assert np.array_equal(buf[:, :, :w], oracle.gpuorder_conv99x11(yc, w1, b1, w2, b2)), (w, h)
            o2 = np.empty((h, w), np.uint8)
            gpu_ctx.conv55([buf[k, :, :w] for k in range(32)], o2, w3, b3)
            assert np.array_equal(o2, m_out), (w, h)


def test_exact_mode_batch_on_device(gpu_ctx, weights_blob):
    """SRCNN_MODE_EXACT on a device-resident batch (frames run one by one through a single
    32-plane workspace): every frame bit-identical to the reference arithmetic."""
    import torch
    n, h, w = 4, 50, 170
    frames = synth_batch(w, h, n, first_frame=30)
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.zeros_like(d_in)
    d_pre = torch.zeros((n, h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.set_mode(S.MODE_EXACT)
    try:
        gpu_ctx.forward_y_dev(d_in.data_ptr(), w, h * w, d_out.data_ptr(), w, h * w, w, h, n, d_pre.data_ptr())
        gpu_ctx.synchronize()
    finally:
        gpu_ctx.set_mode(S.MODE_MFMA)
    out, pre = d_out.cpu().numpy(), d_pre.cpu().numpy()
    for k in range(n):
        r_out, r_pre = oracle.forward_y(frames[k], weights_blob)
        assert np.array_equal(out[k], r_out) and np.array_equal(pre[k], r_pre)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_weights_all_modes(gpu_ctx, weights_blob, seed):
    """The weight tables are caller data (srcnn_set_weights): random models of the same shape
    and magnitude go through every packing path -- MFMA fragments (bitwise against the FMA-order
    model), the exact kernels (bitwise against the reference arithmetic) and the split-f16
    fragments (tolerance; the mode accepts them because its range check passes)."""
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
        gpu_ctx.set_weights_blob(blob)
        pre = np.empty(y.shape, np.float32)
        out = gpu_ctx.forward_y(y, preclamp=pre)
        assert np.array_equal(pre, m_pre) and np.array_equal(out, m_out)
        assert np.abs(pre - r_pre).max() <= TOL_PRE_ABS * scale
        gpu_ctx.set_mode(S.MODE_EXACT)
        e_pre = np.empty(y.shape, np.float32)
        e_out = gpu_ctx.forward_y(y, preclamp=e_pre)
        assert np.array_equal(e_pre, r_pre) and np.array_equal(e_out, r_out)
        gpu_ctx.set_mode(S.MODE_SPLIT16)
        s_pre = np.empty(y.shape, np.float32)
        s_out = gpu_ctx.forward_y(y, preclamp=s_pre)
        assert np.abs(s_pre - r_pre).max() <= TOL_PRE_ABS * scale
        assert np.abs(s_out.astype(int) - r_out.astype(int)).max() <= 1
    finally:
        gpu_ctx.set_mode(S.MODE_MFMA)
        gpu_ctx.set_weights_blob(weights_blob)


def test_launch_geometry_reported_by_query_plan(gpu_ctx):
    """A lone 3840x2160 plane: 30 strips of 128 output columns (column seams, no halo columns) cut into
    2 x n_CU work items; a batch keeps the regular strip x segment grid over the same 30 strips."""
    one = gpu_ctx.query_plan(3840, 2160, 1)
    assert one["strips"] == 30 and one["workgroups"] % 2 == 0 and one["workgroups"] >= 256
    batch = gpu_ctx.query_plan(3840, 2160, 64)       # a large batch: regular strip x segment x frame grid
    assert batch["strips"] == 30 and batch["workgroups"] == 30 * batch["segments"] * 64
    small = gpu_ctx.query_plan(3840, 2160, 8)        # a small batch repeats the plane's work items frame after frame
    assert small["strips"] == 30 and small["workgroups"] == 8 * one["workgroups"]
    narrow = gpu_ctx.query_plan(130, 700, 1)        # last strip would hold 2 columns: halo columns instead
    assert narrow["strips"] == 2


def test_query_plan_reports_what_was_launched():
    """srcnn_query_plan and run_strip() take the launch geometry from one value (strip_geometry()).  For every case of
    tests/golden/make_query_plan_pins.py -- six plane sizes in MODE_MFMA, MODE_REFBYTES and MODE_SPLIT16, 1920x1080 batches either
    side of kItemBatchMax and of the per-frame launches, the two per-layer launches -- a child process bound to the tuning build
    launches, reads the geometry of the last launch through srcnn_debug_last_launch_plan (six numbers, then the launch's
    frames) and asks query_plan.  The launch is the one pinned from the library as it was before (query_plan_pins.json, taken
    on 256 compute units); the report equals the launch (its workgroups are those of the whole batch); and the report equals
    the pinned report except where the fixture lists a corrected one: the hand-kept mirror reported the float32 kernel's LDS
    size in MODE_SPLIT16.  The per-layer launches have no report of their own: query_plan describes the fused pass."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    golden = Path(__file__).resolve().parent / "golden"
    r = subprocess.run([sys.executable, str(golden / "make_query_plan_pins.py"), "--print"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = json.loads((golden / "query_plan_pins.json").read_text())
    assert got["n_cu"] == want["n_cu"] == 256 and len(got["cases"]) == len(want["cases"]) == 27
    for g, w in zip(got["cases"], want["cases"]):
        case = (w["call"], w["mode"], w["width"], w["height"], w["frames"])
        assert case == (g["call"], g["mode"], g["width"], g["height"], g["frames"])
        q, l = g["query_plan"], g["launch"]
        assert l == w["launch"], (case, l, w["launch"])
        assert q == w.get("corrected_query_plan", w["query_plan"]), (case, q, w)
        if g["call"].startswith("forward_y"):
            assert q[1:] == l[1:6] and q[0] * l[6] == l[0] * g["frames"], (case, q, l)
