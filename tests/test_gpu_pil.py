"""Pillow's resize of uint8 images on the GPU (srcnn_resize_pil_image_dev and the calls built on it): the bytes equal the numpy
restatement (tests/pil_reference.py) and Pillow's own committed results (tests/golden/pil_resize_golden.npz) on every listed
shape, for both filters, in every layout; both kernel forms agree; the process calls equal their two-call compositions."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.torch_api import compile_module
import pil_reference as R
from test_gpu_resize_f32 import make_module

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "pil_resize_golden.npz"
SENTINEL = 0xA5
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(shape, channels):
    """The source of a shape, (2, channels, H, W) bytes made of the three inputs of pil_reference.inputs, and per filter the
    restatement's result and Pillow's committed one, composed the same way.  Computed once, never written to."""
    sh, sw, dh, dw = shape
    ins = R.inputs(sh, sw)
    key = f"out/{sh}x{sw}-{dh}x{dw}"
    pick = {1: [("random",), ("checker",)],
            3: [("extremes0", "extremes1", "extremes2"), ("random", "checker", "random")],
            4: [("random", "checker", "extremes0", "extremes1"), ("extremes2", "random", "checker", "checker")]}[channels]

    def plane(name, table):
        return table(name[:8])[..., int(name[8])] if name.startswith("extremes") else table(name)
    src = np.stack([np.stack([plane(n, lambda k: ins[k]) for n in frame]) for frame in pick])
    out = {}
    for fname, f in R.FILTERS.items():
        ref = np.stack([np.stack([R.resize(p, dh, dw, f) for p in frame]) for frame in src])
        pil = np.stack([np.stack([plane(n, lambda k: golden()[f"{key}/{k}/{fname}"]) for n in frame]) for frame in pick])
        out[fname] = (ref, pil)
    src.setflags(write=False)
    return src, out


class Bytes:
    """(n, c, h, w) bytes inside a sentinel-filled device buffer: planar (px_step 1) or interleaved (px_step max(c, 3), channel
    pitch 1), with row strides and pitches larger than the plane and the first element one byte off the buffer's base."""

    def __init__(self, kind, n, c, h, w, scale=1.0):
        if kind == "planar":
            px, stride = 1, w + 5
            ch = (h + 1) * stride + 3
            frame = c * ch + 11
        else:
            px = max(c, 3)
            stride, ch = w * px + 7, 1
            frame = (h + 1) * stride + 5
        self.shape, self.steps = (n, c, h, w), (frame, ch, stride, px)
        self.buf = torch.full((1 + n * frame + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.view = self.buf.as_strided(self.shape, self.steps, 1)
        self.image = S.Image(self.buf.data_ptr() + 1, S.ELEM_U8, px, stride, ch, frame, scale)

    def put(self, a):
        self.view.copy_(torch.from_numpy(np.array(a)))      # (a copy: the shared cases are read-only)
        return self

    def get(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside.as_strided(self.shape, self.steps, 1).fill_(False)
        return bool((self.buf[outside] == SENTINEL).all())

    def frame(self, f):
        return S.Image(self.image.ptr + f * self.steps[0], S.ELEM_U8, self.steps[3], self.steps[2], self.steps[1], 0, self.image.scale)


def run(call, *a, **kw):
    torch.cuda.synchronize()
    call(*a, **kw)
    torch.cuda.synchronize()


def resize_dev(ctx, src, dh, dw, fname, skind="planar", dkind="planar"):
    n, c, sh, sw = src.shape
    s, d = Bytes(skind, n, c, sh, sw).put(src), Bytes(dkind, n, c, dh, dw)
    run(ctx.resize_pil_image_dev, s.image, sw, sh, d.image, dw, dh, c, n, R.FILTERS[fname])
    assert d.guards_intact(), "an element outside the destination's planes was written"
    assert s.guards_intact() and np.array_equal(s.get(), src), "the source is read only"
    return d.get()


@pytest.fixture(scope="module")
def pctx():
    ctx = S.Context(0)          # no model: the resize needs none
    yield ctx
    ctx.close()


_tuning = None


def hooks():
    global _tuning
    if _tuning is None:
        _tuning = C.CDLL(str(S.tuning_library_path()))
        prod = S.load_library()
        for name in ("srcnn_create", "srcnn_destroy", "srcnn_last_error", "srcnn_synchronize", "srcnn_resize_pil_image_dev"):
            getattr(_tuning, name).argtypes = getattr(prod, name).argtypes
            getattr(_tuning, name).restype = getattr(prod, name).restype
        _tuning.srcnn_debug_resample_pil_limits.argtypes = [C.POINTER(C.c_int)]
        _tuning.srcnn_debug_resample_pil_form.argtypes = [C.c_int]
    return _tuning


@pytest.fixture()
def tctx():
    """A context of the tuning library, where srcnn_debug_resample_pil_form reaches; the hook is put back afterwards."""
    lib = hooks()
    ctx = object.__new__(S.Context)
    ctx._lib, h = lib, C.c_void_p()
    assert lib.srcnn_create(C.byref(h), 0) == 0
    ctx._h, ctx.device = h, 0
    yield ctx
    lib.srcnn_debug_resample_pil_form(-1)
    ctx.close()


# ---- every shape, both filters, every layout: the restatement's bytes and Pillow's -------------------------------------------
@pytest.mark.parametrize("shape", R.all_shapes(), ids=ids)
def test_bitwise_on_every_shape_filter_and_layout(pctx, shape):
    sh, sw, dh, dw = shape
    src, want = case(shape, 3)
    for fname in R.FILTERS:
        ref, pil = want[fname]
        assert np.array_equal(ref, pil), "the restatement and Pillow's committed bytes agree (tests/test_pil_cpu.py)"
        for skind in ("planar", "hwc"):
            for dkind in ("planar", "hwc"):
                got = resize_dev(pctx, src, dh, dw, fname, skind, dkind)
                diff = (got != pil).mean()
                assert diff == 0.0, f"{fname} {skind} -> {dkind}: {diff:.3%} of the bytes differ from Pillow's"


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("shape", [(23, 37, 46, 74), (61, 97, 20, 32), (9, 200, 9, 13), (33, 65, 16, 257)], ids=ids)
def test_one_and_four_channels(pctx, shape, channels):
    """1 channel interleaved is one channel of an H x W x 3 picture (px_step 3); 4 channels interleaved is RGBA."""
    src, want = case(shape, channels)
    for fname in R.FILTERS:
        for skind, dkind in (("hwc", "planar"), ("planar", "hwc")):
            assert np.array_equal(resize_dev(pctx, src, shape[2], shape[3], fname, skind, dkind), want[fname][1]), (fname, skind)


def test_two_frames_against_one_frame_at_a_time(pctx):
    shape = (23, 37, 69, 111)
    src, want = case(shape, 3)
    s, d = Bytes("hwc", 2, 3, 23, 37).put(src), Bytes("hwc", 1, 3, 69, 111)
    for f in range(2):
        run(pctx.resize_pil_image_dev, s.frame(f), 37, 23, d.image, 111, 69, 3, 1, S.PIL_BICUBIC)
        assert np.array_equal(d.get()[0], want["bicubic"][1][f]) and d.guards_intact(), f


def test_the_scale_of_a_descriptor_is_ignored(pctx):
    src, want = case((23, 37, 46, 74), 1)
    s, d = Bytes("planar", 2, 1, 23, 37, scale=0.0).put(src), Bytes("planar", 2, 1, 46, 74, scale=float("nan"))
    run(pctx.resize_pil_image_dev, s.image, 37, 23, d.image, 74, 46, 1, 2, S.PIL_BICUBIC)
    assert np.array_equal(d.get(), want["bicubic"][1])


# ---- the two kernel forms -----------------------------------------------------------------------------------------------------
def last_form():
    return hooks().srcnn_debug_resample_pil_last_form()


def test_both_forms_are_hit_each_side_of_the_ratio_bound_and_agree(tctx):
    lib = hooks()
    out = (C.c_int * 6)()
    assert lib.srcnn_debug_resample_pil_limits(out) == 0
    tr, tc, hc, ratio, kmax, rmax = list(out)
    assert (tr, tc, hc) == tuple(R.tile_bounds()[k] for k in ("PIL_TR", "PIL_TC", "PIL_HC")) and ratio == 4
    rng = np.random.default_rng(5)
    lib.srcnn_debug_resample_pil_form(-1)
    # rows at the bound and one beyond it, then columns
    for shape, form in (((ratio * 19, 50, 19, 50), 1), ((ratio * 19 + 1, 50, 19, 50), 0), ((30, ratio * 21, 30, 21), 1),
                        ((30, ratio * 21 + 1, 30, 21), 0), ((23, 37, 46, 74), 1), ((9, 200, 9, 13), 0), ((40, 31, 1, 1), 0)):
        sh, sw, dh, dw = shape
        src = rng.integers(0, 256, (1, 2, sh, sw), dtype=np.uint8)
        want = np.stack([R.resize(p, dh, dw, R.BICUBIC) for p in src[0]])[None]
        lib.srcnn_debug_resample_pil_form(-1)
        a = resize_dev(tctx, src, dh, dw, "bicubic")
        assert last_form() == form, f"{shape}: expected the {'tiled' if form else 'general'} form"
        assert np.array_equal(a, want), shape
        if form == 1:
            lib.srcnn_debug_resample_pil_form(0)
            b = resize_dev(tctx, src, dh, dw, "bicubic", "hwc", "hwc")
            assert last_form() == 0, "the general form through the hook"
            assert np.array_equal(a, b), f"{shape}: the two forms give different bytes"


@pytest.mark.parametrize("shape", [(23, 37, 35, 55), (64, 64, 129, 127), (61, 97, 30, 48), (5, 7, 10, 7), (17, 19, 17, 19)], ids=ids)
def test_the_general_form_gives_pillows_bytes_where_the_tiled_form_serves(tctx, shape):
    src, want = case(shape, 3)
    hooks().srcnn_debug_resample_pil_form(0)
    for fname in R.FILTERS:
        assert np.array_equal(resize_dev(tctx, src, shape[2], shape[3], fname), want[fname][1]), fname
        assert last_form() == 0


# ---- the grid-walk loops: more planes, rows and row tiles than grid y and z hold -----------------------------
def planes_dev(ctx, planes, n_frames, channels, dh, dw):
    """(n_frames * channels, H, W) packed planar bytes through one call"""
    _, sh, sw = planes.shape
    src = torch.from_numpy(planes).cuda()
    out = torch.full((n_frames * channels, dh, dw), SENTINEL, dtype=torch.uint8, device="cuda")
    s = S.Image(src.data_ptr(), S.ELEM_U8, 1, sw, sh * sw, channels * sh * sw)
    d = S.Image(out.data_ptr(), S.ELEM_U8, 1, dw, dh * dw, channels * dh * dw)
    run(ctx.resize_pil_image_dev, s, sw, sh, d, dw, dh, channels, n_frames, S.PIL_BICUBIC)
    return out.cpu().numpy()


def planes_ref(planes, dh, dw):
    return np.ascontiguousarray(np.moveaxis(R.resize(np.ascontiguousarray(np.moveaxis(planes, 0, 2)), dh, dw), 2, 0))


@pytest.mark.parametrize("form,shape", [("tiled", (2, 3, 4, 5)), ("general", (2, 11, 2, 2))])
@pytest.mark.parametrize("n_frames,channels", [(21846, 3), (65537, 1)], ids=["3x21846", "1x65537"])
def test_more_planes_than_grid_z_holds(tctx, form, shape, n_frames, channels):
    sh, sw, dh, dw = shape
    planes = np.random.default_rng(n_frames).integers(0, 256, (n_frames * channels, sh, sw), dtype=np.uint8)
    hooks().srcnn_debug_resample_pil_form(-1)
    got = planes_dev(tctx, planes, n_frames, channels, dh, dw)
    assert last_form() == (form == "tiled")
    assert np.array_equal(got, planes_ref(planes, dh, dw))


@pytest.mark.parametrize("form,shape", [("tiled", (524289, 3, 1048577, 3)), ("general", (65539, 11, 65537, 2))])
def test_more_rows_and_row_tiles_than_grid_y_holds(tctx, form, shape):
    """tiled: 65,537 row tiles, the last of one row; general: 65,539 source rows in the first launch, 65,537 output rows in the
    second"""
    sh, sw, dh, dw = shape
    planes = np.random.default_rng(sh).integers(0, 256, (1, sh, sw), dtype=np.uint8)
    hooks().srcnn_debug_resample_pil_form(-1)
    got = planes_dev(tctx, planes, 1, 1, dh, dw)
    assert last_form() == (form == "tiled")
    assert np.array_equal(got, planes_ref(planes, dh, dw))


# ---- the table cache ----------------------------------------------------------------------------------------------------------
def test_a_geometry_or_filter_change_rebuilds_the_tables():
    a, b = (23, 37, 46, 74), (61, 97, 30, 48)
    with S.Context(0) as ctx:
        for shape, fname in ((a, "bicubic"), (b, "bicubic"), (a, "bicubic"), (a, "bilinear"), (a, "bicubic"), (b, "bilinear"),
                             ((37, 23, 74, 46), "bicubic"), (a, "bicubic")):
            src, want = case(shape, 3) if shape in (a, b) else (None, None)
            if src is None:      # the transposed geometry: the same numbers, another table
                src = np.ascontiguousarray(np.swapaxes(case(a, 3)[0], 2, 3))
                ref = np.stack([np.stack([R.resize(p, shape[2], shape[3], R.FILTERS[fname]) for p in fr]) for fr in src])
            else:
                ref = want[fname][1]
            assert np.array_equal(resize_dev(ctx, src, shape[2], shape[3], fname), ref), (shape, fname)


# ---- the process calls ----------------------------------------------------------------------------------------------------------
def out_image(kind, n, c, h, w):
    if kind == "u8":
        t = torch.zeros((n, h, w, c), dtype=torch.uint8, device="cuda")
        return t, S.Image(t.data_ptr(), S.ELEM_U8, c, w * c, 1, h * w * c, 255.0)
    t = torch.zeros((n, c, h, w), dtype=torch.float32, device="cuda")
    return t, S.Image(t.data_ptr(), S.ELEM_F32, 1, w, h * w, c * h * w)


@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("mode", [S.MODE_MFMA, S.MODE_BANDED16], ids=["mfma", "banded16"])
@pytest.mark.parametrize("channels,f2", [(1, 3), (3, 1)], ids=["1ch-9-3-5", "3ch-9-1-5"])
def test_process_pil_equals_resize_then_forward(channels, f2, mode, out):
    shape = (23, 37, 46, 74)
    sh, sw, dh, dw = shape
    src, want = case(shape, channels)
    fast = compile_module(make_module(channels, f2, "zeros", 11), mode=mode, input_range=1.0)
    try:
        ctx = fast.ctx
        for fname in R.FILTERS:
            s = Bytes("hwc", 2, channels, sh, sw, scale=1.0 / 255.0).put(src)
            one_t, one = out_image(out, 2, channels, dh, dw)
            run(ctx.process_pil_image_dev, s.image, sw, sh, one, dw, dh, 2, R.FILTERS[fname])
            mid = Bytes("planar", 2, channels, dh, dw, scale=1.0 / 255.0)
            two_t, two = out_image(out, 2, channels, dh, dw)
            run(ctx.resize_pil_image_dev, s.image, sw, sh, mid.image, dw, dh, channels, 2, R.FILTERS[fname])
            assert np.array_equal(mid.get(), want[fname][1])
            run(ctx.forward_image_dev, mid.image, two, dw, dh, 2)
            a, b = one_t.cpu().numpy(), two_t.cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), fname
            assert len(np.unique(a)) > 1, "the model wrote a picture, not a constant"
    finally:
        fast.close()


def test_process_rgb_pil_equals_resize_then_process_rgb():
    shape = (23, 37, 46, 74)
    sh, sw, dh, dw = shape
    src, want = case(shape, 3)
    fast = compile_module(make_module(1, 3, "zeros", 12), input_range=1.0)
    try:
        ctx = fast.ctx
        for fname, clamp in (("bicubic", (0.0, 1.0)), ("bilinear", None)):
            s = Bytes("hwc", 2, 3, sh, sw, scale=1.0 / 255.0).put(src)
            for out in ("u8", "f32"):
                one_t, one = out_image(out, 2, 3, dh, dw)
                run(ctx.process_rgb_pil_image_dev, s.image, sw, sh, one, dw, dh, S.LUMA_BT601, clamp, 2, R.FILTERS[fname])
                mid = Bytes("planar", 2, 3, dh, dw, scale=1.0 / 255.0)
                two_t, two = out_image(out, 2, 3, dh, dw)
                run(ctx.resize_pil_image_dev, s.image, sw, sh, mid.image, dw, dh, 3, 2, R.FILTERS[fname])
                run(ctx.process_rgb_image_dev, mid.image, dw, dh, two, dw, dh, S.LUMA_BT601, clamp, 2)
                a, b = one_t.cpu().numpy(), two_t.cpu().numpy()
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (fname, out)
                assert len(np.unique(a)) > 1
    finally:
        fast.close()


# ---- torch ----------------------------------------------------------------------------------------------------------------------
def test_torch_methods():
    shape = (23, 37, 46, 74)
    sh, sw, dh, dw = shape
    src, want = case(shape, 3)
    fast3 = compile_module(make_module(3, 1, "zeros", 13), input_range=1.0)
    fast1 = compile_module(make_module(1, 3, "zeros", 14), input_range=1.0)
    try:
        x = torch.from_numpy(src.copy()).cuda().contiguous(memory_format=torch.channels_last)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            r = fast3.resize_pil(x, (dh, dw))
            z = r.to(torch.int32) + 1                      # the next torch op on that stream consumes the result unsynchronised
            lin = fast3.resize_pil(x, (dh, dw), filter="bilinear")
        stream.synchronize()
        assert r.dtype == torch.uint8 and r.shape == (2, 3, dh, dw) and r.is_contiguous(memory_format=torch.channels_last)
        assert np.array_equal(r.cpu().numpy(), want["bicubic"][0]) and np.array_equal(lin.cpu().numpy(), want["bilinear"][0])
        assert np.array_equal(z.cpu().numpy(), want["bicubic"][0].astype(np.int32) + 1)
        rd = fast3.resize_pil(x.clone(memory_format=torch.preserve_format), (dh, dw))      # the default stream
        planar = fast3.resize_pil(x.contiguous(), (dh, dw))
        down = fast1.resize_pil(r, (sh, sw))             # any channel count, the way down, whatever the module's channels
        torch.cuda.synchronize()
        assert torch.equal(rd, r) and torch.equal(planar, r) and planar.is_contiguous()
        assert np.array_equal(down.cpu().numpy(), np.stack([np.stack([R.resize(p, sh, sw) for p in f]) for f in want["bicubic"][0]]))
        one = fast3.resize_pil(x[1], (dh, dw))
        assert one.shape == (3, dh, dw) and torch.equal(one, r[1])
        # upscale_pil = forward_image(resize_pil), upscale_rgb_pil = upscale_rgb_image(resize_pil) at the same size
        for kw in ({}, {"out_dtype": torch.float32, "out_channels_last": False}, {"filter": "bilinear", "out_dtype": torch.float16}):
            f = {"filter": kw["filter"]} if "filter" in kw else {}
            rest = {k: v for k, v in kw.items() if k != "filter"}
            a = fast3.upscale_pil(x, scale=2, **kw)
            b = fast3.forward_image(fast3.resize_pil(x, (dh, dw), **f), **rest)
            assert a.dtype == b.dtype and a.stride() == b.stride() and torch.equal(a, b), kw
            a = fast1.upscale_rgb_pil(x, size=(dh, dw), clamp=(0.0, 1.0), **kw)
            b = fast1.upscale_rgb_image(fast1.resize_pil(x, (dh, dw), **f), size=(dh, dw), clamp=(0.0, 1.0), **rest)
            assert a.dtype == b.dtype and a.stride() == b.stride() and torch.equal(a, b), kw
        with pytest.raises(TypeError, match=r"resize\(\.\.\., antialias=True\)"):
            fast3.resize_pil(x.float(), (dh, dw))
    finally:
        fast3.close()
        fast1.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusals_leave_the_context_usable(pctx):
    shape = (23, 37, 46, 74)
    sh, sw, dh, dw = shape
    src, want = case(shape, 3)
    s, d = Bytes("planar", 2, 3, sh, sw).put(src), Bytes("planar", 2, 3, dh, dw)
    call = pctx.resize_pil_image_dev
    f32 = torch.zeros((2, 3, dh, dw), dtype=torch.float32, device="cuda")
    as_f32 = S.Image(f32.data_ptr(), S.ELEM_F32, 1, dw, dh * dw, 3 * dh * dw)
    as_f16 = S.Image(s.image.ptr + 1, S.ELEM_F16, 1, s.steps[2] // 2, s.steps[1] // 2, s.steps[0] // 2)
    folded = S.Image(d.image.ptr, S.ELEM_U8, 1, dw, dw, d.steps[0], 1.0)                      # channel pitch inside the plane
    over = S.Image(s.image.ptr + 7, S.ELEM_U8, 1, dw, dh * dw, 3 * dh * dw, 1.0)              # destination over the source
    null = S.Image(0, S.ELEM_U8, 1, dw, dh * dw, 3 * dh * dw, 1.0)
    B = S.PIL_BICUBIC
    for bad in (lambda: call(s.image, sw, sh, as_f32, dw, dh, 3, 2, B), lambda: call(as_f16, sw, sh, d.image, dw, dh, 3, 2, B),
                lambda: call(s.image, sw, sh, d.image, dw, dh, 3, 2, 1), lambda: call(s.image, sw, sh, d.image, dw, dh, 3, 2, 0),
                lambda: call(s.image, sw, sh, d.image, dw, dh, 3, 2, 4), lambda: call(s.image, sw, sh, folded, dw, dh, 3, 2, B),
                lambda: call(s.image, sw, sh, over, dw, dh, 3, 2, B), lambda: call(s.image, sw, sh, null, dw, dh, 3, 2, B),
                lambda: call(null, sw, sh, d.image, dw, dh, 3, 2, B), lambda: call(s.image, sw, 0, d.image, dw, dh, 3, 2, B),
                lambda: call(s.image, sw, sh, d.image, 0, dh, 3, 2, B), lambda: call(s.image, sw, sh, d.image, dw, dh, 0, 2, B),
                lambda: call(s.image, sw, sh, d.image, dw, dh, 3, 0, B)):
        assert "resize_pil_image_dev" in _err(bad, S.ERR_INVALID)
        d.view.fill_(0)
        run(call, s.image, sw, sh, d.image, dw, dh, 3, 2, B)
        assert np.array_equal(d.get(), want["bicubic"][1]) and d.guards_intact(), "a good call on the same context after the refusal"
    # no model: the process calls are refused with the state error, the resize still runs
    out_t, out = out_image("u8", 2, 3, dh, dw)
    _err(lambda: pctx.process_pil_image_dev(s.image, sw, sh, out, dw, dh, 2, B), S.ERR_STATE)
    _err(lambda: pctx.process_rgb_pil_image_dev(s.image, sw, sh, out, dw, dh, S.LUMA_BT601, None, 2, B), S.ERR_STATE)
    run(call, s.image, sw, sh, d.image, dw, dh, 3, 2, B)
    assert np.array_equal(d.get(), want["bicubic"][1])


def test_process_refusals_leave_the_context_usable():
    shape = (23, 37, 46, 74)
    sh, sw, dh, dw = shape
    src, _ = case(shape, 3)
    fast3 = compile_module(make_module(3, 1, "zeros", 15), input_range=1.0)
    fast1 = compile_module(make_module(1, 1, "zeros", 16), input_range=1.0)
    try:
        s = Bytes("hwc", 2, 3, sh, sw, scale=1.0 / 255.0).put(src)
        f32src = torch.zeros((2, 3, sh, sw), dtype=torch.float32, device="cuda")
        as_f32 = S.Image(f32src.data_ptr(), S.ELEM_F32, 1, sw, sh * sw, 3 * sh * sw)
        out_t, out = out_image("u8", 2, 3, dh, dw)
        small_t, small = out_image("u8", 2, 3, sh - 1, dw)
        B = S.PIL_BICUBIC
        p3, rgb1, rgb3 = fast3.ctx.process_pil_image_dev, fast1.ctx.process_rgb_pil_image_dev, fast3.ctx.process_rgb_pil_image_dev
        L = S.LUMA_BT601

        def raw(src_im, dst_im, luma, clamp, height):      # past the Python layer's own checks, to the library's
            c1 = fast1.ctx
            c1._check(c1._lib.srcnn_process_rgb_pil_image_dev(c1._h, C.byref(src_im.c()), sw, sh, C.byref(dst_im.c()), dw, height,
                                                              (C.c_float * 4)(*luma), (C.c_float * 2)(*clamp) if clamp else None, 2, B))
        good3 = fast3.upscale_pil(torch.from_numpy(src.copy()).cuda(), scale=2)
        good1 = fast1.upscale_rgb_pil(torch.from_numpy(src.copy()).cuda(), scale=2)
        torch.cuda.synchronize()
        for ctx, bad, code in ((fast3.ctx, lambda: p3(as_f32, sw, sh, out, dw, dh, 2, B), S.ERR_INVALID),
                               (fast3.ctx, lambda: p3(s.image, sw, sh, out, dw, dh, 2, 1), S.ERR_INVALID),
                               (fast3.ctx, lambda: p3(s.image, sw, sh, small, dw, sh - 1, 2, B), S.ERR_INVALID),
                               (fast3.ctx, lambda: rgb3(s.image, sw, sh, out, dw, dh, L, None, 2, B), S.ERR_STATE),
                               (fast1.ctx, lambda: rgb1(as_f32, sw, sh, out, dw, dh, L, None, 2, B), S.ERR_INVALID),
                               (fast1.ctx, lambda: rgb1(s.image, sw, sh, out, dw, dh, L, None, 2, 5), S.ERR_INVALID),
                               (fast1.ctx, lambda: raw(s.image, out, (0.0, 0.0, 0.0, 0.0), None, dh), S.ERR_INVALID),
                               (fast1.ctx, lambda: raw(s.image, out, L, (1.0, 0.0), dh), S.ERR_INVALID),
                               (fast1.ctx, lambda: raw(s.image, small, L, None, sh - 1), S.ERR_INVALID)):
            _err(bad, code)
            assert torch.equal(fast3.upscale_pil(torch.from_numpy(src.copy()).cuda(), scale=2), good3)
            assert torch.equal(fast1.upscale_rgb_pil(torch.from_numpy(src.copy()).cuda(), scale=2), good1)
        fast3.ctx.set_mode(S.MODE_EXACT)      # the gate of srcnn_process_image_dev: MODE_MFMA and MODE_BANDED16 only
        _err(lambda: p3(s.image, sw, sh, out, dw, dh, 2, B), S.ERR_STATE)
        fast3.ctx.set_mode(S.MODE_MFMA)
        assert torch.equal(fast3.upscale_pil(torch.from_numpy(src.copy()).cuda(), scale=2), good3)
    finally:
        fast3.close()
        fast1.close()
