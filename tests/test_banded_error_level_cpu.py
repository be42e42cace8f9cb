"""The float32 error level (tests/error_level.py) without a GPU: the bound can fail, and its shapes follow the kernels' tiles.

The numpy model of the split arithmetic (tests/test_banded16_cpu.py::split_model; tests/test_wide16_cpu.py for 128 / 64) passes
error_level.check -- the very assertion, with the very numbers, that tests/test_gpu_banded_error_level.py applies to the kernels
-- and the same model with ONE seeded defect fails it, for every defect, in every 64 / 32 case of the GPU test, on the same pooled
shapes.  Switching a defect on and reading the assertion that rejects it is the demonstration of the GPU test's sensitivity.

Every case uses generator seed 0 (none had to be changed to separate a defect from the intact model)."""
import re

import numpy as np
import pytest

import error_level as E
import test_banded16_cpu as B16
import test_wide16_cpu as W16

PADDINGS = ["replicate", "zero"]


# ---- the seeded defects -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_intact_split_model_is_inside_and_every_defect_is_outside(channels, f2, padding):
    plain, _, images, y = E.narrow_case(channels, f2, padding, False)
    tables = B16.host_tables(plain)
    run = lambda defect: [B16.split_model(x, plain, padding, 3, defect, tables) for x in images]
    what = f"{channels}ch 9-{f2}-5 {padding}"
    E.check(run(None), y, f"{what} split model")
    for defect in B16.DEFECTS:
        outs = run(defect)
        with pytest.raises(AssertionError):                    # (prints the defect's line)
            E.check(outs, y, f"{what} {defect}")
        r_max, _ = E.ratios(outs, y)
        assert r_max > E.MAX_FACTOR, f"{what}: the defect {defect} passes the max bound ({r_max:.2f} x Y_max)"


def test_the_defects_change_what_they_say():
    """Each defect is a strict part of the next larger one: one tap's w_lo of all w_lo (f2 > 1), one K step's a_lo of all a_lo,
    one unit's lo terms of hi-only; and a 1 x 1 model has one tap, so there the two w_lo defects are one."""
    plain, _, images, _ = E.narrow_case(1, 3, "replicate", False)
    x = images[-2]
    tables = B16.host_tables(plain)
    outs = {d: B16.split_model(x, plain, "replicate", 3, d, tables) for d in (None,) + B16.DEFECTS}
    for a in outs:
        for b in outs:
            assert a == b or not np.array_equal(outs[a], outs[b]), (a, b)
    hi_only = B16.split_model(x, plain, "replicate", 1, None, tables)
    right = np.arange(x.shape[2]) % 64 >= 32
    assert right.any() and np.array_equal(outs["lo_right_unit"][:, :, 40:60], hi_only[:, :, 40:60])      # (5 columns from a unit's edge)
    assert np.array_equal(outs["lo_right_unit"][:, :, 5:27], outs[None][:, :, 5:27])
    plain1 = E.narrow_case(1, 1, "replicate", False)[0]
    t1 = B16.host_tables(plain1)
    assert np.array_equal(B16.split_model(x, plain1, "replicate", 3, "w_lo", t1), B16.split_model(x, plain1, "replicate", 3, "w_lo_one_tap", t1))


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("f2", [1, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_wide_split_model_is_inside_and_hi_parts_alone_are_outside(channels, f2, padding):
    model, images, y = E.wide_case(channels, 128, f2, 64, padding, False)
    key = ("error level", channels, f2)
    run = lambda terms: [W16.split_model(x, model, key, padding, terms) for x in images]
    what = f"128/64 {channels}ch 9-{f2}-5 {padding}"
    E.check(run(3), y, f"{what} split model")
    outs = run(1)
    with pytest.raises(AssertionError):
        E.check(outs, y, f"{what} hi parts alone")
    assert E.ratios(outs, y)[0] > E.MAX_FACTOR


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def test_factors_are_those_of_the_rule():
    assert (E.MAX_FACTOR, E.RMS_FACTOR) == (4.0, 3.0)


def test_yardstick_is_pooled_and_at_the_float32_level():
    """Y is a property of the model and the data: pooled over the shapes it is some float32 ulps of the output (values near 60 to
    200: 4e-6 to 1.5e-5 per ulp), hundreds of times below pre_tolerance, and the same for the byte and the integer-float forms."""
    _, model, images, y = E.narrow_case(1, 3, "replicate", False)
    assert len(images) == len(E.SHAPES) == len(y.refs) and all(r.dtype == np.float64 for r in y.refs)
    assert 0 < y.rms < y.max < 1e-4
    again = E.yardstick(model, "replicate", E.float_images(images, False))
    assert again.max == y.max and again.rms == y.rms and all(np.array_equal(a, b) for a, b in zip(again.refs, y.refs))
    # the reference itself passes its own bound at the factor 1, and a shifted one does not pass at 4
    f32 = [E.forward(x, model, "replicate", E.torch.float32) for x in images]
    assert f32[0].dtype == np.float32
    assert E.ratios(f32, y) == pytest.approx((1.0, 1.0))
    with pytest.raises(AssertionError):
        E.check([r + 5 * y.max for r in y.refs], y, "a shifted reference")
    # the [0, 1] case is the same model in other units: references within float32 rounding of W1 * 255 and x / 255
    _, _, _, yu = E.narrow_case(1, 3, "replicate", True)
    assert max(np.abs(a - b).max() for a, b in zip(yu.refs, y.refs)) < 1e-3
    assert 0.25 * y.max < yu.max < 4 * y.max


# ---- the shapes ---------------------------------------------------------------------------------------------------------------
def test_shapes_follow_the_tile_constants_of_the_kernel_unit():
    """A change of a tile size breaks this test instead of silently un-covering the edges."""
    text = E.KERNEL_UNIT.read_text()
    k = {n: int(re.search(rf"^constexpr int [^;]*\b{n} = (\d+)\b", text, flags=re.M).group(1)) for n in E.TILE_NAMES}
    assert k == E.tile_constants()
    assert "SL3_OUT = SL3_COLS - 4" in text and "blockIdx.x * SL1_COLS" in text and "blockIdx.x * SL2_COLS" in text
    assert "tx * SL3_OUT - 2 + c" in text and "if (tile >= n_tiles) return;" in text
    widths, heights = {w for w, _ in E.SHAPES}, {h for _, h in E.SHAPES}
    for cols in (k["SL1_COLS"], k["SL2_COLS"], k["SL3_COLS"] - 4):
        assert {cols - 1, cols, cols + 1} <= widths, cols
    for rows in (k["SL1_ROWS"], k["SL2_ROWS"], k["SL3_SEG"]):
        assert {rows - 1, rows, rows + 1} <= heights, rows
    assert {1, 2, 3} <= widths
    tiles = [E.l3_tiles(w, h, k) for w, h in E.SHAPES]
    xcds = k["SL3_XCDS"]
    assert any(t > xcds and t % xcds for t in tiles), "a tile count beyond one round that leaves blocks without a tile"
    assert any(t % xcds == 0 for t in tiles) and any(t < xcds for t in tiles)
    assert all(w * h < 10000 for w, h in E.SHAPES) and len(set(E.SHAPES)) == len(E.SHAPES)
    assert set(E.SHORT_SHAPES) <= set(E.SHAPES) and (1, 1) in E.SHORT_SHAPES
    for cols in (k["SL1_COLS"], k["SL2_COLS"], k["SL3_COLS"] - 4):
        assert cols in {w for w, _ in E.SHORT_SHAPES}


def test_shapes_for_the_present_tiles():
    assert E.tile_constants() == dict(SL1_COLS=128, SL1_ROWS=8, SL2_COLS=64, SL2_ROWS=16, SL3_COLS=128, SL3_SEG=16, SL3_XCDS=8)
    assert set(E.SHAPES) >= {(1, 1), (3, 3), (63, 7), (64, 8), (65, 9), (124, 15), (125, 16), (127, 17), (128, 16), (129, 17), (249, 33)}
    assert E.SHAPES == [(1, 1), (2, 5), (3, 3), (63, 7), (64, 8), (65, 9), (123, 15), (124, 15), (125, 16), (127, 17), (128, 16),
                        (129, 17), (249, 33), (125, 49)]
    assert E.SHORT_SHAPES == [(1, 1), (64, 8), (124, 15), (128, 16)]


def test_shapes_move_with_the_tiles():
    k = dict(E.tile_constants(), SL2_COLS=32, SL3_SEG=8, SL1_ROWS=4)
    s = E.shapes(k)
    assert {31, 32, 33} <= {w for w, _ in s} and {3, 4, 5, 7, 8, 9, 15, 16, 17} <= {h for _, h in s}
    assert 64 not in {w for w, _ in s}
