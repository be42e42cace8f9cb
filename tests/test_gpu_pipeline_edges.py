"""GPU tests of the byte kernels around the conv path (srcnn_cpp_amd/csrc/srcnn_pipeline.hip) where
tests/test_gpu_pipeline.py does not reach: the column split of the resize's vertical pass (float32 below dw - dw % 8, fixed
point in the tail) on planes where the two passes differ in whole rows, the tiled4 and fused kernels with a tail, the shapes
at and one past every limit of the kernel selection, the table cache under alternating geometries, the colour kernels on all
2^24 inputs, and srcnn_process_bgr_dev with padded strides.  BIT-EXACT against oracle/opencv_steps.c throughout, the product
library only; which kernel a shape reaches, and that the tie inputs tell the two passes apart, is asserted without a device in
tests/test_resize_geometry_cpu.py."""
import numpy as np
import pytest

import oracle
import srcnn_cpp_amd as S
from pipeline_reference import (PIPELINE_CASES, SHAPES, chroma_tie_image, discriminating, tie_phase, tie_plane, visible_step)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sw,sh,dw,dh,kernel,wants_tie", SHAPES)
def test_resize_table_rows_bit_exact(gpu_ctx, sw, sh, dw, dh, kernel, wants_tie):
    rng = np.random.default_rng(sw + 7 * dw + 131 * sh)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    assert np.array_equal(gpu_ctx.resize_cubic(src, dw, dh), oracle.resize_cubic(src, dw, dh))
    if wants_tie:
        tie = tie_plane(sw, sh, tie_phase(sh, dh))
        # what this guards, from the reference: the picture of record steps at column dw - dw % 8 on this plane, and a kernel
        # with one pass for every column, or the split elsewhere, gets at least 8 pixels wrong on either side of it
        assert visible_step(tie, dw, dh) >= 1
        assert min(discriminating(tie, dw, dh)) >= 8
        assert np.array_equal(gpu_ctx.resize_cubic(tie, dw, dh), oracle.resize_cubic(tie, dw, dh))


def test_table_cache_alternating_geometries(gpu_ctx):
    """ensure_tables() keeps one set of tables keyed on (sw, sh, dw, dh): A, B, A, then C with B's (dw, dh) but another
    source size, then B again -- every result from the tables of its own geometry."""
    a, b, c = (40, 64, 60, 96), (48, 100, 60, 125), (50, 90, 60, 125)
    rng = np.random.default_rng(5)
    for sw, sh, dw, dh in (a, b, a, c, b):
        src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        assert np.array_equal(gpu_ctx.resize_cubic(src, dw, dh), oracle.resize_cubic(src, dw, dh)), (sw, sh, dw, dh)


def test_colour_kernels_on_every_input(gpu_ctx):
    """Both conversions are integer maps of 2^24 triples: all of them, as 4096 x 4096 pictures."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    c0, c1, c2 = [((v >> s) & 255).astype(np.uint8) for s in (0, 8, 16)]
    bgr = np.stack([c0, c1, c2], axis=2)
    for got, want in zip(gpu_ctx.bgr2ycrcb(bgr), oracle.bgr2ycrcb(bgr)):
        assert np.array_equal(got, want)
    assert np.array_equal(gpu_ctx.ycrcb2bgr(c0, c1, c2), oracle.ycrcb2bgr(c0, c1, c2))


def pipeline_input(w, h, name):
    if name == "noise":        # random bytes per channel: cubic overshoot and out-of-gamut triples reach every sat8
        return np.random.default_rng(w + 1000 * h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if name == "grey-tie":     # B = G = R = tie_plane: Y ties, chroma flat at 128
        return np.repeat(tie_plane(w, h, 1)[:, :, None], 3, axis=2)
    return chroma_tie_image(w, h, {"cr-tie": 1, "cb-tie": 2}[name])


# noise everywhere; the three tie pictures on the fused x1.5 cases (x1.5 has rows of vertical phase 1/2)
PIPELINE_RUNS = [(w, h, scale, size, fused, name) for w, h, scale, size, fused in PIPELINE_CASES
                 for name in ("noise", "grey-tie", "cr-tie", "cb-tie") if name == "noise" or (fused and scale == 1.5)]


@pytest.mark.parametrize("w,h,scale,size,fused,name", PIPELINE_RUNS)
def test_whole_pipeline_with_a_tail(gpu_ctx, weights_blob, w, h, scale, size, fused, name):
    """The two fused launches (bgr_to_y_resized_kernel, resize_merge_kernel) at output widths of 4 x an odd number -- the
    mixed branch of vpass4 -- and one unfused neighbour per limit.  As tests/test_gpu_pipeline.py::test_whole_pipeline:
    SRCNN_MODE_EXACT equals the reference arithmetic, the MFMA mode the FMA-order model, both bitwise."""
    bgr = pipeline_input(w, h, name)
    assert S.scaled_size(w, h, scale) == oracle.scaled_size(w, h, scale) == size
    ref = oracle.process_bgr(bgr, scale, weights_blob)
    if name != "noise":
        # from the reference alone: on this picture an all-fixed-point vertical pass shows in the output
        fixed = oracle.process_bgr(bgr, scale, weights_blob, vertical=oracle.VERTICAL_FIXED)
        assert (fixed != ref).any(axis=2).sum() >= 8
        comp = {"grey-tie": 0, "cr-tie": 1, "cb-tie": 2}[name]
        assert min(discriminating(oracle.bgr2ycrcb(bgr)[comp], *size)) >= 8
    out = gpu_ctx.process_bgr(bgr, scale)
    gpu_ctx.set_mode(S.MODE_EXACT)
    try:
        exact = gpu_ctx.process_bgr(bgr, scale)
    finally:
        gpu_ctx.set_mode(S.MODE_MFMA)
    assert np.array_equal(exact, ref)
    assert np.array_equal(out, oracle.process_bgr(bgr, scale, weights_blob, y_path=oracle.gpuorder_forward_y))


@pytest.mark.parametrize("out_pad,why", [(8, "dword-aligned rows: the two fused launches"),
                                         (7, "unaligned rows: the three separate kernels")])
def test_process_bgr_dev_padded_strides(gpu_ctx, out_pad, why):
    import torch
    w, h, scale = 40, 64, 1.5
    ow, oh = S.scaled_size(w, h, scale)
    guard, fill = 64, 0xA5
    rng = np.random.default_rng(77)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    sstride, dstride = 3 * w + 5, 3 * ow + out_pad
    src = np.full(guard + h * sstride + guard, fill, np.uint8)
    src_rows = src[guard:guard + h * sstride].reshape(h, sstride)
    src_rows[:, :3 * w] = bgr.reshape(h, 3 * w)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((guard + oh * dstride + guard,), fill, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    gpu_ctx.process_bgr_dev(d_in.data_ptr() + guard, sstride, w, h, scale, d_out.data_ptr() + guard, dstride)
    gpu_ctx.synchronize()
    got = d_out.cpu().numpy()
    rows = got[guard:guard + oh * dstride].reshape(oh, dstride)
    assert np.array_equal(rows[:, :3 * ow].reshape(oh, ow, 3), gpu_ctx.process_bgr(bgr, scale))
    assert (rows[:, 3 * ow:] == fill).all() and (got[:guard] == fill).all() and (got[-guard:] == fill).all()
    assert np.array_equal(d_in.cpu().numpy(), src)
