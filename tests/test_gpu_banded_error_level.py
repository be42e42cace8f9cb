"""Every kernel form of the banded path (srcnn_spatial.cpp, srcnn_spatial_kernels.hip) held to the float32 error level of
tests/error_level.py, at the tile bounds of its three kernels (error_level.SHAPES), and guard elements around the outputs of the
64 / 32 device entry points.

Forms: 1 and 3 channels x f2 = 1, 3, 5 x replicate and zero padding x SRCNN_MODE_MFMA (layer 2 in float32) and SRCNN_MODE_BANDED16
(layer 2 in split f16), as bytes (forward_y / forward_color with preclamp=), as integer-valued floats and as [0, 1] floats with
set_input_range(1) (forward_f32); the one form that does not run banded -- 1 channel, 9-1-5, replicate, MODE_MFMA, bytes: the
strip path, which has a bitwise model -- is left out.  Wide models (128 / 64 and 100 / 40 filters) with set_wide_split16 off and
on run the short shape list.

Per plane max |out - ref64| <= 4 Y_max, pooled over the case's planes rms <= 3 Y_rms (error_level.check: the assertion that
tests/test_banded_error_level_cpu.py shows to reject every seeded defect of the split arithmetic), and for bytes
assert_u8_consistent at 4 Y_max.  Y is the deviation of torch's float32 evaluation on the CPU from its float64 one: never a GPU
mode.  Each case prints its max / Y_max and rms / Y_rms (DESIGN.md holds the table of one run)."""
import numpy as np
import pytest
import torch

import error_level as E
import srcnn_cpp_amd as S
from spatial_reference import assert_u8_consistent
from test_gpu_wide import run_f32, run_u8

pytestmark = pytest.mark.gpu

PADDINGS = ["replicate", "zero"]
MODES = [S.MODE_MFMA, S.MODE_BANDED16]
MODE_NAMES = {S.MODE_MFMA: "MFMA", S.MODE_BANDED16: "BANDED16"}
FORMS = [(c, f2, p, m) for c in (1, 3) for f2 in (1, 3, 5) for p in PADDINGS for m in MODES]
BYTE_FORMS = [f for f in FORMS if f != (1, 1, "replicate", S.MODE_MFMA)]          # (that one runs the strip kernels)
form_id = lambda f: f"{f[0]}ch-9{f[1]}5-{f[2]}-{MODE_NAMES[f[3]]}"


@pytest.fixture(scope="module")
def ectx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(ectx):
    def reset():
        ectx.set_mode(S.MODE_MFMA)
        ectx.set_padding("replicate")
        ectx.set_input_range(255.0)
        ectx.set_wide_split16(False)
    reset()
    yield
    reset()


def check_bytes(ctx, images, y, what):
    results = [run_u8(ctx, x) for x in images]
    E.check([pre for _, pre in results], y, what)
    for (out, _), ref in zip(results, y.refs):
        assert_u8_consistent(out, ref, E.MAX_FACTOR * y.max)


# ---- the 64 / 32 forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", BYTE_FORMS, ids=form_id)
def test_bytes_are_at_the_float32_level(ectx, form):
    channels, f2, padding, mode = form
    plain, _, images, y = E.narrow_case(channels, f2, padding, False)
    ectx.set_model(*plain)
    ectx.set_padding(padding)
    ectx.set_mode(mode)
    assert (ectx.model_channels(), ectx.model_f2()) == (channels, f2)
    check_bytes(ectx, images, y, f"bytes {form_id(form)}")


@pytest.mark.parametrize("unit", [False, True], ids=["integers", "unit-range"])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_floats_are_at_the_float32_level(ectx, form, unit):
    channels, f2, padding, mode = form
    plain, _, images, y = E.narrow_case(channels, f2, padding, unit)
    ectx.set_model(*plain)
    ectx.set_padding(padding)
    ectx.set_mode(mode)
    ectx.set_input_range(1.0 if unit else 255.0)
    images = images if unit else E.float_images(images, False)
    assert all(x.dtype == np.float32 and np.abs(x).max() <= ectx.input_range() for x in images)
    E.check([run_f32(ectx, x) for x in images], y, f"floats {'[0, 1]' if unit else 'integers'} {form_id(form)}")


# ---- the wide forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["f32", "split16"])
@pytest.mark.parametrize("f2", [1, 5])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n1,n2", [(128, 64), (100, 40)])
def test_wide_models_are_at_the_float32_level(ectx, n1, n2, channels, f2, split):
    ectx.set_wide_split16(split)
    for padding in PADDINGS:
        ectx.set_padding(padding)
        for unit in (False, True):
            model, images, y = E.wide_case(channels, n1, f2, n2, padding, unit)
            ectx.set_model(*model)
            assert ectx.model_shape() == (channels, n1, f2, n2)
            ectx.set_input_range(1.0 if unit else 255.0)
            what = f"{n1}/{n2} {channels}ch 9-{f2}-5 {padding} {'split16' if split else 'f32'}"
            if not unit:
                check_bytes(ectx, images, y, f"bytes {what}")
            floats = images if unit else E.float_images(images, False)
            E.check([run_f32(ectx, x) for x in floats], y, f"floats {'[0, 1]' if unit else 'integers'} {what}")


# ---- guard elements around the outputs of the 64 / 32 device entry points -----------------------------------------------------
GUARD_SHAPES = [(65, 9), (125, 16), (129, 17)]
LEAD = 64                  # guard elements in front of the destination


def _layout(w, h, channels, interleaved, spare):
    """(row stride, channel pitch, frame pitch) in elements, all larger than the plane needs (rows by `spare` elements)."""
    stride = (channels * w if interleaved else w) + spare
    ch = 0 if interleaved or channels == 1 else stride * h + 9
    frame = (stride * h if interleaved or channels == 1 else channels * ch) + 13
    return stride, ch, frame


def _place(buf, frames, layout, interleaved, lead=0):
    """Write frames ([C, h, w] each) into the flat buffer by the layout; returns the mask of the elements written."""
    stride, ch, frame = layout
    mask = np.zeros(buf.size, bool)
    for k, x in enumerate(frames):
        c, h, w = x.shape
        rows = np.moveaxis(x, 0, 2).reshape(1, h, c * w) if interleaved else x
        for p in range(rows.shape[0]):
            for r in range(h):
                o = lead + k * frame + p * ch + r * stride
                buf[o:o + rows.shape[2]] = rows[p, r]
                mask[o:o + rows.shape[2]] = True
    return mask


@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES.get)
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("entry", ["y", "color", "f32-1ch", "f32-3ch"])
def test_device_entry_points_write_inside_the_plane_only(ectx, entry, padding, mode):
    """Row strides and frame pitches larger than the plane, a sentinel in the whole destination (and in front of it): every
    element outside [h, w] of a frame still holds it, and inside are the values of the host call, bit for bit."""
    channels = 3 if entry in ("color", "f32-3ch") else 1
    floats, interleaved = entry.startswith("f32"), entry == "color"
    plain, _, _, _ = E.narrow_case(channels, 3, padding, False)
    ectx.set_model(*plain)
    ectx.set_padding(padding)
    ectx.set_mode(mode)
    n = 2
    for w, h in GUARD_SHAPES:
        frames = E.byte_images(channels, 3, [(w, h)]) + E.byte_images(channels, 4, [(w, h)])
        if floats:
            frames = [x * np.float32(0.5) + np.float32(0.25) for x in E.float_images(frames, False)]      # non-integers in range
        src_l, dst_l = _layout(w, h, channels, interleaved, 7), _layout(w, h, channels, interleaved, 10)
        src = np.full(n * src_l[2], 7, frames[0].dtype)           # (what lies in the source's padding must not be read either)
        _place(src, frames, src_l, interleaved)
        size = LEAD + n * dst_l[2] + LEAD
        if floats:
            want = [run_f32(ectx, x) for x in frames]
            sentinel = np.float32(-12345.0)
        else:
            results = [run_u8(ectx, x) for x in frames]
            want, want_pre = [r[0] for r in results], [r[1] for r in results]
            sentinel, pre_sentinel = np.uint8(0xA5), np.float32(-7.5)
            d_pre = torch.full((size,), float(pre_sentinel), dtype=torch.float32, device="cuda")
        expect = np.full(size, sentinel)
        inside = _place(expect, want, dst_l, interleaved, LEAD)
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.full((size,), sentinel.item(), dtype=torch.float32 if floats else torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if floats:
            ectx.forward_f32_dev(d_src.data_ptr(), src_l[0], src_l[1], src_l[2], d_dst.data_ptr() + 4 * LEAD, dst_l[0], dst_l[1],
                                 dst_l[2], w, h, n)
        else:
            call = ectx.forward_color_dev if interleaved else ectx.forward_y_dev
            call(d_src.data_ptr(), src_l[0], src_l[2], d_dst.data_ptr() + LEAD, dst_l[0], dst_l[2], w, h, n, d_pre.data_ptr() + 4 * LEAD)
        ectx.synchronize()
        got = d_dst.cpu().numpy()
        assert (got[~inside] == sentinel).all(), f"{entry} {w}x{h}: elements outside the plane were written"
        assert np.array_equal(got[inside], expect[inside]), f"{entry} {w}x{h}: not the values of the host call"
        assert inside.sum() == n * channels * w * h and not inside[:LEAD].any() and not inside[-LEAD:].any()
        if not floats:
            expect_pre = np.full(size, pre_sentinel)
            _place(expect_pre, want_pre, dst_l, interleaved, LEAD)
            got_pre = d_pre.cpu().numpy()
            assert (got_pre[~inside] == pre_sentinel).all(), f"{entry} {w}x{h}: pre-clamp floats outside the plane were written"
            assert np.array_equal(got_pre[inside], expect_pre[inside])
