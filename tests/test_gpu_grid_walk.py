"""The grid-walk loops: every float, stored-image, antialiased-resize and metric kernel launches with grid y and z capped at
65,535 and walks the planes, rows and row tiles that lie beyond (`for (z = blockIdx.z; z < n_planes; z += gridDim.z)`).  Each
case here makes one grid dimension exceed the cap, so that a workgroup runs a second iteration of one of those loops: the
frame / channel split of a walked plane, the 64-bit offsets at a large z or row, the LDS tiles reused between two tiles of one
workgroup, the reduction buffer reused across planes, the partial-sum index.  Walked counts are no multiple of the channel
count or of the tile height; every plane, row and frame holds its own random data; outputs are pre-filled and guarded.
The rules are those of the kernels' own test files (test_gpu_resize_f32, test_gpu_image, test_gpu_resize_aa, test_gpu_metrics):
no tolerance here is new.  The unsigned 8-bit kernels do not walk: a section of its own pins what their entry points do at
65,536 rows.  DESIGN.md 4.17 lists every walk loop with the case that enters it."""
import math

import numpy as np
import pytest
import torch

import oracle
import srcnn_cpp_amd as S
from srcnn_cpp_amd.torch_api import compile_module
import image_reference as IR
import metrics_reference as RM
import resize_aa_reference as RA
import resize_f32_reference as RF
from test_gpu_image import Buf, load_model, run, u8_scale_for, varied
from test_gpu_metrics import check, loaded, measure, pair, tile, u64
from test_gpu_resize_aa import model as aa_model32, tiled as aa_tiled
from test_gpu_resize_f32 import make_module, same_bits, tiled as f32_tiled

pytestmark = pytest.mark.gpu

CAP = 65535                                                   # grid y and z of every launch: the hardware's limit
BATCHES = {"3ch-x-21846": (21846, 3), "1ch-x-65537": (65537, 1)}      # (frames, channels): 65,538 and 65,537 planes
F32_RT, AA_TR = 16, 16                                        # output rows of a tile; test_gpu_resize_f32 / _aa assert them against the hooks
BY_NAME = {f[0]: f for f in IR.FORMATS}
PLANAR_F16 = ("planar-f16", IR.F16, "planar")


@pytest.fixture(scope="module")
def wctx():
    ctx = S.Context(0)          # no model: resizes and metrics need none
    yield ctx
    ctx.close()


def f32_call(entry, x, dh, dw):
    """srcnn_resize_cubic_f32_dev or srcnn_resize_cubic_aa_f32_dev on a contiguous CUDA tensor (N, C, H, W); the output lies between
    two guard frames of NaN, which must come back untouched -> (N, C, dh, dw)"""
    n, c, h, w = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32
    buf = torch.full((n + 2, c, dh, dw), float("nan"), dtype=torch.float32, device=x.device)
    out = buf[1:n + 1]
    run(entry, x.data_ptr(), w, h * w, c * h * w, w, h, out.data_ptr(), dw, dh * dw, c * dh * dw, dw, dh, c, n)
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[n + 1]).all(), "the frames either side of the output stay untouched"
    assert not torch.isnan(out).any(), "every output element is written"
    return out


def under_the_cap(entry, x, dh, dw):
    """The same planes in two calls of which neither reaches the cap"""
    n, c = x.shape[:2]
    half = n // 2
    assert (n - half) * c <= CAP
    return torch.cat([f32_call(entry, x[:half], dh, dw), f32_call(entry, x[half:], dh, dw)])


def within(got, ref, tol, x, what):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bound = tol * float(np.abs(x).max())
    print(f"{what}: |got - ref64| = {err:.3g} (bound {bound:.3g}) over all {got.size} values")
    assert err <= bound


# ---- plane walks (grid z): tiny planes -----------------------------------------------------------------------------------------
F32_PLANE = {"direct": (7, 5, 4, 3), "tiled": (4, 5, 8, 10)}


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", F32_PLANE)
def test_resize_f32_walks_planes(wctx, form, batch):
    """srcnn_resize_cubic_f32_dev, grid z: every plane against ref64 (the reference takes all planes at once), and bitwise against
    the same planes in two calls under the cap."""
    (n, c), (sh, sw, dh, dw) = BATCHES[batch], F32_PLANE[form]
    assert n * c > CAP
    assert f32_tiled(sh, sw, dh, dw) == (form == "tiled")
    x = RF.uniform((n, c, sh, sw), n + sh)
    xd = torch.from_numpy(x).cuda()
    got = f32_call(wctx.resize_cubic_f32_dev, xd, dh, dw)
    within(got.cpu().numpy(), RF.ref64(x, dh, dw), RF.TOL, x, f"{form} {sh}x{sw} -> {dh}x{dw}, {n * c} planes")
    assert same_bits(got, under_the_cap(wctx.resize_cubic_f32_dev, xd, dh, dw))


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", F32_PLANE)
def test_resize_image_walks_planes(wctx, form, batch):
    """srcnn_resize_cubic_image_dev, grid z: interleaved bytes in, planar float16 out, rows and frames padded, both buffers one
    element off their base.  store(the float32 call(load(x))), bit for bit."""
    (n, c), (sh, sw, dh, dw) = BATCHES[batch], F32_PLANE[form]
    assert n * c > CAP and f32_tiled(sh, sw, dh, dw) == (form == "tiled")
    bits = np.random.default_rng(n + dw).integers(0, 256, (n, c, sh, sw)).astype(np.uint8)
    scale = 1.0 / 255.0
    ref = f32_call(wctx.resize_cubic_f32_dev, torch.from_numpy(IR.load(bits, IR.U8, scale)).cuda(), dh, dw).cpu().numpy()
    s = Buf(BY_NAME["interleaved-u8"], n, c, sh, sw, scale, off=1, row_pad=3, frame_pad=7).put(bits)
    d = Buf(PLANAR_F16, n, c, dh, dw, 1.0, off=1, row_pad=5, frame_pad=7)
    run(wctx.resize_cubic_image_dev, s.image, sw, sh, d.image, dw, dh, c, n)
    assert IR.same_stored(d.get(), IR.store(ref, IR.F16), IR.F16)
    assert d.guards_intact() and s.guards_intact()


AA_PLANE = {"tiled": (8, 10, 4, 5), "general": (11, 5, 2, 1)}


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", AA_PLANE)
def test_resize_aa_f32_walks_planes(wctx, form, batch):
    """srcnn_resize_cubic_aa_f32_dev, grid z; the general form also indexes its workspace with the walked plane (z * sh * dw).
    Bitwise against the float32 model on the library's tables, within TOL of ref64, and bitwise against two calls under the cap:
    all planes, each of them."""
    (n, c), (sh, sw, dh, dw) = BATCHES[batch], AA_PLANE[form]
    assert n * c > CAP and aa_tiled(sh, sw, dh, dw) == (form == "tiled")
    x = RA.uniform((n, c, sh, sw), n + sw)
    xd = torch.from_numpy(x).cuda()
    got = f32_call(wctx.resize_cubic_aa_f32_dev, xd, dh, dw)
    assert same_bits(got, aa_model32(x, dh, dw))
    within(got.cpu().numpy(), RA.ref64(x, dh, dw), RA.TOL, x, f"aa {form} {sh}x{sw} -> {dh}x{dw}, {n * c} planes")
    assert same_bits(got, under_the_cap(wctx.resize_cubic_aa_f32_dev, xd, dh, dw))


@pytest.mark.parametrize("batch", BATCHES)
def test_resize_aa_image_general_walks_planes(wctx, batch):
    """srcnn_resize_cubic_aa_image_dev, general form, grid z: planar bfloat16 in, interleaved bytes out."""
    (n, c), (sh, sw, dh, dw) = BATCHES[batch], AA_PLANE["general"]
    assert n * c > CAP and not aa_tiled(sh, sw, dh, dw)
    bits = IR.store(np.random.default_rng(n + 1).random((n, c, sh, sw), dtype=np.float32), IR.BF16)
    ref = f32_call(wctx.resize_cubic_aa_f32_dev, torch.from_numpy(IR.load(bits, IR.BF16)).cuda(), dh, dw).cpu().numpy()
    s = Buf(BY_NAME["planar-bf16"], n, c, sh, sw, 1.0, off=1, row_pad=3, frame_pad=5).put(bits)
    d = Buf(BY_NAME["interleaved-u8"], n, c, dh, dw, 255.0, off=1, row_pad=2, frame_pad=3)
    run(wctx.resize_cubic_aa_image_dev, s.image, sw, sh, d.image, dw, dh, c, n)
    want = IR.store(ref, IR.U8, 255.0)
    assert IR.same_stored(d.get(), want, IR.U8) and len(np.unique(want)) > 16
    assert d.guards_intact() and s.guards_intact()


def batch_reference(a, b, **kw):
    """metrics_reference on every plane, the frames taken 8,192 at a time"""
    return np.concatenate([RM.metrics_batch(loaded(a[f:f + 8192]), loaded(b[f:f + 8192]), **kw) for f in range(0, a.shape[0], 8192)])


METRIC_PLANE = [("sse", 1, 1), ("sse", 3, 5), ("sse+ssim", 11, 11), ("sse+ssim", 12, 13)]


def metric_walk(ctx, n, c, rh, rw, what, luma):
    flags = S.METRIC_SSE | (S.METRIC_SSIM if "ssim" in what else 0)
    per_frame = 1 if luma is not None else c
    assert n * per_frame > CAP
    a, b = pair((n, c, rh, rw), n + rh * rw)
    got = measure(ctx, a, b, luma=luma, flags=flags)
    assert got.shape == (n, per_frame, 4)
    check(got, batch_reference(a, b, luma=luma, ssim="ssim" in what), f"{what} {rh} x {rw}, {n * per_frame} planes")
    walked = sorted({0} | {z // per_frame for z in range(CAP, n * per_frame)})
    assert len(walked) >= 2
    for f in walked:
        one = measure(ctx, a[f:f + 1], b[f:f + 1], luma=luma, flags=flags)
        assert np.array_equal(u64(one[0]), u64(got[f])), f"frame {f} alone equals frame {f} of the batch"


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("what,rh,rw", METRIC_PLANE, ids=lambda v: str(v))
def test_metrics_walk_planes(wctx, what, rh, rw, batch):
    """srcnn_metrics_image_dev, grid z of the SSE and SSIM kernels and grid x of the finish: the reduction buffer reused from plane
    to plane, the partials at z * n_sse + k and z * n_ssim + ...; every plane against the reference."""
    n, c = BATCHES[batch]
    metric_walk(wctx, n, c, rh, rw, what, None)


def test_metrics_luma_walks_planes(wctx):
    """65,537 frames of 3 channels measured on their luma: one plane per frame, the walked ones read three channels at a walked
    frame's offset."""
    metric_walk(wctx, 65537, 3, 12, 13, "sse+ssim", RM.LUMA_BT601)


# ---- row walks (grid y): one narrow plane --------------------------------------------------------------------------------------
F32_ROWS = {"direct": (131078, 6, 65539, 3), "tiled": (524289, 3, 1048577, 6)}


def f32_rows_geometry(form):
    sh, sw, dh, dw = F32_ROWS[form]
    assert f32_tiled(sh, sw, dh, dw) == (form == "tiled")
    if form == "tiled":
        assert -(-dh // F32_RT) == 65537 > CAP and dh % F32_RT == 1, "65,537 row tiles, the last of one row"
    else:
        assert dh > CAP
    return sh, sw, dh, dw


@pytest.mark.parametrize("form", F32_ROWS)
def test_resize_f32_walks_rows(wctx, form):
    """srcnn_resize_cubic_f32_dev, grid y: output rows (direct) or row tiles (tiled, hbuf and sbuf reused by the workgroup that
    takes tile 0 and tile 65,535) beyond the cap.  Every value against ref64."""
    sh, sw, dh, dw = f32_rows_geometry(form)
    x = RF.uniform((1, 1, sh, sw), sh)
    got = f32_call(wctx.resize_cubic_f32_dev, torch.from_numpy(x).cuda(), dh, dw)
    within(got.cpu().numpy(), RF.ref64(x, dh, dw), RF.TOL, x, f"{form} {sh}x{sw} -> {dh}x{dw}")


@pytest.mark.parametrize("form", F32_ROWS)
def test_resize_image_walks_rows(wctx, form):
    """srcnn_resize_cubic_image_dev, grid y: float16 in, bytes out, both one channel of an interleaved picture (px_step 3)."""
    sh, sw, dh, dw = f32_rows_geometry(form)
    bits = IR.store(np.random.default_rng(dh).random((1, 1, sh, sw), dtype=np.float32), IR.F16)
    ref = f32_call(wctx.resize_cubic_f32_dev, torch.from_numpy(IR.load(bits, IR.F16)).cuda(), dh, dw).cpu().numpy()
    oscale = u8_scale_for(ref)
    s = Buf(BY_NAME["interleaved-f16"], 1, 1, sh, sw, 1.0, off=1, row_pad=1).put(bits)
    d = Buf(BY_NAME["interleaved-u8"], 1, 1, dh, dw, oscale, off=1, row_pad=2)
    assert s.image.px_step == 3 and d.image.px_step == 3
    run(wctx.resize_cubic_image_dev, s.image, sw, sh, d.image, dw, dh, 1, 1)
    want = IR.store(ref, IR.U8, oscale)
    assert IR.same_stored(d.get(), want, IR.U8) and varied(want)
    assert d.guards_intact() and s.guards_intact()


AA_ROWS = {"tiled": (2097154, 4, 1048577, 2), "general": (327695, 11, 65539, 2)}


@pytest.mark.parametrize("form", AA_ROWS)
def test_resize_aa_f32_walks_rows(wctx, form):
    """srcnn_resize_cubic_aa_f32_dev, grid y: 65,537 row tiles (tiled: hbuf reused), or the horizontal launch over 327,695 source
    rows and the vertical one over 65,539 output rows (general).  Bitwise against the float32 model, within TOL of ref64."""
    sh, sw, dh, dw = AA_ROWS[form]
    assert aa_tiled(sh, sw, dh, dw) == (form == "tiled")
    if form == "tiled":
        assert -(-dh // AA_TR) == 65537 > CAP and dh % AA_TR == 1
    else:
        assert sh > CAP and dh > CAP
    x = RA.uniform((1, 1, sh, sw), dh)
    got = f32_call(wctx.resize_cubic_aa_f32_dev, torch.from_numpy(x).cuda(), dh, dw)
    assert same_bits(got, aa_model32(x, dh, dw))
    within(got.cpu().numpy(), RA.ref64(x, dh, dw), RA.TOL, x, f"aa {form} {sh}x{sw} -> {dh}x{dw}")


@pytest.mark.parametrize("width", [1, 5])
def test_forward_image_converts_65539_rows_both_ways(width):
    """srcnn_forward_image_dev with bytes in and out around the smallest 1-channel model: convert_image_kernel runs once into the
    packed float32 planes and once out of them, each time over 65,539 rows.  Width 1 is the narrowest picture the model's gate
    admits (the element path); width 5 adds a run of four and its tail.  store(forward_f32_dev(load(x))), bit for bit."""
    h, w = 65539, width
    assert h > CAP
    fast = compile_module(make_module(1, 1, "zeros", 3), input_range=2.0)
    try:
        ctx = fast.ctx
        bits = np.random.default_rng(w).integers(0, 256, (1, 1, h, w)).astype(np.uint8)
        scale = 1.0 / 255.0
        xd = torch.from_numpy(IR.load(bits, IR.U8, scale)).cuda()
        out = torch.full((1, 1, h, w), float("nan"), dtype=torch.float32, device="cuda")
        run(ctx.forward_f32_dev, xd.data_ptr(), w, h * w, h * w, out.data_ptr(), w, h * w, h * w, w, h, 1)
        ref = out.cpu().numpy()
        assert np.isfinite(ref).all()
        oscale = u8_scale_for(ref)
        s = Buf(BY_NAME["interleaved-u8"], 1, 1, h, w, scale, off=1, row_pad=2).put(bits)
        d = Buf(BY_NAME["interleaved-u8"], 1, 1, h, w, oscale, off=1, row_pad=1)
        run(ctx.forward_image_dev, s.image, d.image, w, h, 1)
        want = IR.store(ref, IR.U8, oscale)
        assert np.array_equal(d.get(), want) and varied(want)
        assert d.guards_intact() and s.guards_intact()
    finally:
        fast.close()


@pytest.mark.parametrize("tail", ["periodic", "distinct-tail"])
def test_ssim_walks_bands(wctx, tail):
    """srcnn_metrics_image_dev, grid y of the SSIM kernel: 11 columns x (64 x 65,536 + 11) rows of bytes are 65,537 bands of one
    column tile, of which the last two are walked.
    periodic: the pair repeats with the band height in its rows (two unrelated random 64 x 11 blocks), so every full band sees
    the same 74 source rows and the picture's sum is 65,536 S(74 x 11) + S(11 x 11): both S from metrics_reference, added in
    math.fsum (tests/test_metrics_cpu.py holds the reference to this identity on 5 bands); the means agree within SSIM_TOL.
    distinct-tail: the rows of the two walked bands, past the ten they share with the band before, are random data of their own,
    and the expected sum is 65,535 S(74 x 11) + S(those 75 rows).
    The mean over 4,194,305 windows hardly moves when two bands are misread, so both cases also hold the call to the library's
    own sums under the cap: the first 65,535 bands and the last two, measured as pictures of their own, give partial sums that
    are the same bits as the whole picture's (a band's sum depends on its rows alone), and the totals differ only by the order
    in which the finish adds them: at most 265 additions deep (257 of a thread's stride-256 pass, 8 of the tree) in each of
    three sums, on partials whose absolute sum is at most n_win: 3 * 265 * 2^-53 * n_win = 3.7e-7.  With the distinct tail a
    walked band read from any other place sees other random rows, and its 64 window values move by far more than that."""
    T, B = tile()
    k, w = 65536, 11
    rows = k * B + RM.WIN
    cut = (k - 1) * B                                        # the first source row of band 65,535, the first walked one
    assert -(-(rows - RM.WIN + 1) // B) == k + 1 > CAP and w - RM.WIN + 1 <= T and cut // B == CAP
    rng = np.random.default_rng(41)
    blocks = [rng.integers(0, 256, (B, w), dtype=np.uint8) for _ in range(2)]
    host = [RM.periodic_rows(x, rows).copy() for x in blocks]
    if tail == "distinct-tail":
        for x in host:
            x[cut + RM.WIN - 1:] = rng.integers(0, 256, (rows - cut - RM.WIN + 1, w), dtype=np.uint8)
    a, b = (torch.from_numpy(x[None, None]).cuda() for x in host)
    got = measure(wctx, a, b, flags=S.METRIC_SSIM)
    # the reference: one full band of the periodic part, and what closes the picture
    la, lb = (RM.load(x[:B + RM.WIN - 1])[None] for x in host)
    band = RM.metrics(la, lb, sse=False)[0]
    n_full, rest = (k, rows - RM.WIN) if tail == "periodic" else (k - 1, cut)
    last = RM.metrics(RM.load(host[0][rest:])[None], RM.load(host[1][rest:])[None], sse=False)[0]
    n_win = float(k * B + 1)
    assert band[3] == B and n_full * B + last[3] == n_win
    want_sum = math.fsum([band[2]] * n_full + [last[2]])
    assert got.shape == (1, 1, 4) and got[0, 0, 3] == n_win and (got[0, 0, :2] == 0).all()
    err = abs(got[0, 0, 2] / n_win - want_sum / n_win)
    # the library's own sums under the cap
    head = measure(wctx, a[:, :, :cut + RM.WIN - 1], b[:, :, :cut + RM.WIN - 1], flags=S.METRIC_SSIM)
    walked = measure(wctx, a[:, :, cut:], b[:, :, cut:], flags=S.METRIC_SSIM)
    assert head[0, 0, 3] == CAP * B and walked[0, 0, 3] == B + 1 and head[0, 0, 3] + walked[0, 0, 3] == n_win
    check(walked, np.stack([RM.metrics(RM.load(host[0][cut:])[None], RM.load(host[1][cut:])[None], sse=False)]), "the two walked bands alone")
    split = abs(got[0, 0, 2] - (head[0, 0, 2] + walked[0, 0, 2]))
    print(f"{k + 1} bands, {tail}: |mean SSIM - reference| = {err:.3g}; |sum - (65,535 bands + 2 bands)| = {split:.3g}")
    assert err <= RM.SSIM_TOL
    assert split <= 3 * 265 * 2.0 ** -53 * n_win


# ---- the unsigned 8-bit entry points at 65,536 rows: the reference's bytes, or a refusal that launches nothing ------------------
SENTINEL = 0xA5


def bytes_or_refusal(ctx, what, call, outs, wants):
    """call() -> status, writing into the sentinel-filled arrays `outs`: success with the oracle's bytes, or a non-zero status
    with a message and every output byte still the sentinel"""
    for o in outs:
        o.fill(SENTINEL)
    rc = call()
    if rc == 0:
        print(f"{what}: runs")
        for o, want in zip(outs, wants()):
            assert np.array_equal(o, want), f"{what}: success, and not the reference's bytes"
        return True
    msg = ctx._lib.srcnn_last_error(ctx._h).decode()
    print(f"{what}: refused ({rc}): {msg}")
    assert msg and all((o == SENTINEL).all() for o in outs), f"{what}: a refused call writes nothing"
    return False


def u8p(a):
    return a.ctypes.data_as(S._u8p)


@pytest.mark.parametrize("rows", [65535, 65536])
def test_u8_colour_conversions_at_the_grid_limit(wctx, rows):
    """srcnn_bgr2ycrcb and srcnn_ycrcb2bgr take one row per block of grid y and do not walk: 65,535 rows run, 65,536 are refused
    before the launch."""
    lib, h, w = wctx._lib, wctx._h, 2
    rng = np.random.default_rng(rows)
    bgr = rng.integers(0, 256, (rows, w, 3), dtype=np.uint8)
    planes = [np.empty((rows, w), np.uint8) for _ in range(3)]
    ran = bytes_or_refusal(wctx, f"bgr2ycrcb, {rows} rows", lambda: lib.srcnn_bgr2ycrcb(h, u8p(bgr), 3 * w, w, rows, *map(u8p, planes), w),
                           planes, lambda: oracle.bgr2ycrcb(bgr))
    assert ran or rows > CAP
    src = [rng.integers(0, 256, (rows, w), dtype=np.uint8) for _ in range(3)]
    out = np.empty((rows, w, 3), np.uint8)
    ran = bytes_or_refusal(wctx, f"ycrcb2bgr, {rows} rows", lambda: lib.srcnn_ycrcb2bgr(h, *map(u8p, src), w, w, rows, u8p(out), 3 * w),
                           [out], lambda: [oracle.ycrcb2bgr(*src)])
    assert ran or rows > CAP
    small = rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    for got, want in zip(wctx.bgr2ycrcb(small), oracle.bgr2ycrcb(small)):
        assert np.array_equal(got, want), "an ordinary call afterwards gives the usual bytes"
    few = [np.ascontiguousarray(p[:9]) for p in src]
    assert np.array_equal(wctx.ycrcb2bgr(*few), oracle.ycrcb2bgr(*few))


U8_RESIZE = {"tiled4 x2": (32768, 2, 65536, 4), "tiled x2, odd stride": (32768, 3, 65536, 6), "direct /2": (131072, 4, 65536, 2),
             "direct, 65,535 rows": (131070, 4, 65535, 2)}


@pytest.mark.parametrize("case", U8_RESIZE)
def test_u8_resize_at_the_grid_limit(wctx, case):
    """srcnn_resize_cubic to 65,536 rows: the tiled forms take 32 or 8 rows per block and run; the direct form takes one row per
    block and is refused before the launch (at 65,535 rows it runs)."""
    sh, sw, dh, dw = U8_RESIZE[case]
    lib, h = wctx._lib, wctx._h
    src = np.random.default_rng(sh + sw).integers(0, 256, (sh, sw), dtype=np.uint8)
    out = np.empty((dh, dw), np.uint8)
    ran = bytes_or_refusal(wctx, f"resize_cubic, {case}", lambda: lib.srcnn_resize_cubic(h, u8p(src), sw, sw, sh, u8p(out), dw, dw, dh),
                           [out], lambda: [oracle.resize_cubic(src, dw, dh)])
    assert ran or dh > CAP
    small = np.ascontiguousarray(src[:23, :2])
    assert np.array_equal(wctx.resize_cubic(small, 5, 40), oracle.resize_cubic(small, 5, 40)), "an ordinary call afterwards"


# ---- the row-tile walk of the two kernels around a 1-channel model (srcnn_process_rgb_f32_dev) ---------------------------------
def test_process_rgb_f32_walks_row_tiles():
    """luma_resize_f32_kernel and resize_merge_f32_kernel walk row tiles like the plain tiled resize, the second with three fills
    of sbuf per tile; a public call reaches the walk only with a model pass over 1,048,577 rows.  The smallest model (9-1-5) on
    the narrowest tiled geometry of test_resize_f32_walks_rows; bit for bit the composition of the existing calls, as
    tests/test_gpu_rgb_f32.py states it."""
    import test_gpu_rgb_f32 as G
    from rgb_f32_reference import BT601_FULL, merge_f32, rgb
    sh, sw, dh, dw = f32_rows_geometry("tiled")
    luma = BT601_FULL.luma()
    with S.Context(0) as ctx:
        load_model(ctx, 1, 1, "zero", S.MODE_MFMA)      # 9-1-5 for [0, 1] data
        x = rgb((3, sh, sw), 7)
        u, yup, ysr, g = G.composed(ctx, x, dh, dw, luma)
        assert np.isfinite(ysr).all() and len(np.unique(ysr)) > 1000, "the model's output is no constant"
        got = G.rgb_dev(ctx, G.dev(x)[None], dh, dw, luma)[0].cpu().numpy()
        assert not np.isnan(got).any()
        assert G.same_bits(got, merge_f32(u, ysr, yup, g))


@pytest.mark.parametrize("dst", ["interleaved-u8", "planar-bf16"])
def test_process_rgb_image_walks_row_tiles(dst):
    """The accessor forms of the same two kernels (srcnn_process_rgb_image_dev): interleaved bytes in; interleaved bytes out take
    the merge kernel's pixel order, a planar destination its channel passes.  store(process_rgb_f32_dev(load(x))), bit for bit."""
    import test_gpu_rgb_f32 as G
    from rgb_f32_reference import BT601_FULL
    sh, sw, dh, dw = f32_rows_geometry("tiled")
    luma, clamp = BT601_FULL.luma(), (0.0, 1.0)
    with S.Context(0) as ctx:
        load_model(ctx, 1, 1, "zero", S.MODE_MFMA)      # 9-1-5 for [0, 1] data
        bits = np.random.default_rng(9).integers(0, 256, (1, 3, sh, sw)).astype(np.uint8)
        scale = 1.0 / 255.0
        ref = G.rgb_dev(ctx, torch.from_numpy(IR.load(bits, IR.U8, scale)).cuda(), dh, dw, luma, clamp).cpu().numpy()
        assert np.isfinite(ref).all()
        s = Buf(BY_NAME["interleaved-u8"], 1, 3, sh, sw, scale, off=1, row_pad=3).put(bits)
        d = Buf(BY_NAME[dst], 1, 3, dh, dw, 255.0, off=1, row_pad=5)
        run(ctx.process_rgb_image_dev, s.image, sw, sh, d.image, dw, dh, luma, clamp, 1)
        want = IR.store(ref, d.elem, 255.0)
        assert IR.same_stored(d.get(), want, d.elem) and len(np.unique(want)) > 16
        assert d.guards_intact() and s.guards_intact()
