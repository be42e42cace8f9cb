"""The antialiased cubic resize on the GPU (srcnn_resize_cubic_aa_f32(_dev), srcnn_resize_cubic_aa_image_dev,
CompiledModule.resize / resize_image with antialias=True).  The rule under test is bitwise: every kernel form returns the
float32 model of the two passes (tests/resize_aa_reference.py) on the library's own tables, and the image call returns
store(the float32 call(load(x))).  All planes are small."""
import ctypes as C

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.torch_api import compile_module
import image_reference as IR
import resize_aa_reference as R
from test_gpu_image import PLANAR_F32, Buf, run
from test_gpu_resize_f32 import make_module

pytestmark = pytest.mark.gpu

GUARD = float("nan")
TR, TC = 16, 64          # asserted against the hook in test_the_shapes_sit_on_the_tile_and_on_the_bound
TILE_DST = [(TR, TC), (TR + 1, TC + 1), (TR - 1, TC - 1)]
RATIO2 = [(2 * dh, 2 * dw, dh, dw) for dh, dw in TILE_DST]
RATIO4 = [(4 * dh, 4 * dw, dh, dw) for dh, dw in TILE_DST]
BEYOND = [(4 * TR, 4 * TC + 1, TR, TC), (4 * TR + 1, 4 * TC, TR, TC)]      # the general form by one column, by one row
SMALL = [(23, 29, 11, 13), (67, 131, 45, 87)]
THUMBS = [(3, 200, 2, 13), (1, 9, 1, 4), (17, 19, 1, 1)]

_tuning = None


def hooks():
    """The tuning build of the library: the host-only hooks, and (TuningContext) contexts whose calls the form hook steers."""
    global _tuning
    if _tuning is None:
        _tuning = C.CDLL(str(S.tuning_library_path()))
        prod = S.load_library()
        for name in ("srcnn_create", "srcnn_destroy", "srcnn_last_error", "srcnn_synchronize", "srcnn_resize_cubic_aa_f32_dev",
                     "srcnn_resize_cubic_aa_image_dev"):
            getattr(_tuning, name).argtypes = getattr(prod, name).argtypes
            getattr(_tuning, name).restype = getattr(prod, name).restype
        _tuning.srcnn_debug_resample_aa_variant.argtypes = [C.c_int] * 4
        _tuning.srcnn_debug_resample_aa_limits.argtypes = [C.POINTER(C.c_int)]
        _tuning.srcnn_debug_resample_aa_form.argtypes = [C.c_int]
    return _tuning


def tiled(sh, sw, dh, dw):
    return hooks().srcnn_debug_resample_aa_variant(sw, sh, dw, dh) == 1


@pytest.fixture(scope="module")
def actx():
    ctx = S.Context(0)          # no model: the resize needs none
    yield ctx
    ctx.close()


@pytest.fixture()
def tctx():
    """A context of the tuning library, where srcnn_debug_resample_aa_form reaches; the hook is put back afterwards."""
    lib = hooks()
    ctx = object.__new__(S.Context)
    ctx._lib, h = lib, C.c_void_p()
    assert lib.srcnn_create(C.byref(h), 0) == 0
    ctx._h, ctx.device = h, 0
    yield ctx
    lib.srcnn_debug_resample_aa_form(-1)
    ctx.close()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def aa_dev(ctx, x, dh, dw):
    """srcnn_resize_cubic_aa_f32_dev on a contiguous CUDA tensor (N, C, H, W), on the context's own stream."""
    n, c, h, w = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32
    out = torch.full((n, c, dh, dw), GUARD, dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()
    ctx.resize_cubic_aa_f32_dev(x.data_ptr(), w, h * w, c * h * w, w, h, out.data_ptr(), dw, dh * dw, c * dh * dw, dw, dh, c, n)
    ctx.synchronize()
    return out


def aa_plane(ctx, x, dh, dw):
    return aa_dev(ctx, torch.from_numpy(np.array(x, dtype=np.float32))[None, None].cuda(), dh, dw)[0, 0].cpu().numpy()


def model(x, dh, dw):
    """The float32 model on the LIBRARY's tables."""
    sh, sw = x.shape[-2:]
    return R.model32(x, S.cubic_aa_f32_taps(sw, dw), S.cubic_aa_f32_taps(sh, dh))


def plane(sh, sw, seed):
    return R.uniform((sh, sw), seed) * np.float32(2.0) - np.float32(0.5)


# ---- shapes: bitwise against the model ---------------------------------------------------------------------------------------
def test_the_shapes_sit_on_the_tile_and_on_the_bound():
    out = (C.c_int * 5)()
    assert hooks().srcnn_debug_resample_aa_limits(out) == 0
    assert list(out)[:3] == [TR, TC, 4]
    assert all(tiled(*s) for s in SMALL + RATIO2 + RATIO4 + [(9, 11, 18, 22), (5, 7, 5, 7), (1, 9, 1, 4)])
    assert not any(tiled(*s) for s in BEYOND + [(3, 200, 2, 13), (17, 19, 1, 1), (45, 130, 9, 13)])


@pytest.mark.parametrize("sh,sw,dh,dw", SMALL + RATIO2 + RATIO4 + BEYOND + THUMBS, ids=lambda v: str(v))
def test_bitwise_against_the_float32_model(actx, sh, sw, dh, dw):
    x = plane(sh, sw, sh + 3 * dw)
    got = aa_plane(actx, x, dh, dw)
    want = model(x, dh, dw)
    assert got.dtype == np.float32 and got.shape == (dh, dw)
    err = np.abs(got.astype(np.float64) - R.ref64(x, dh, dw)).max()
    print(f"{sh}x{sw} -> {dh}x{dw} ({'tiled' if tiled(sh, sw, dh, dw) else 'general'}): |got - ref64| = {err:.3g}, "
          f"{int((bits(got) != bits(want)).sum())} of {got.size} values differ from the model")
    assert same_bits(got, want)
    assert err <= R.TOL * float(np.abs(x).max())


def test_upscaling_renormalises_the_borders(actx):
    sh, sw, dh, dw = 9, 11, 18, 22
    x = plane(sh, sw, 5)
    got = aa_plane(actx, x, dh, dw)
    assert same_bits(got, model(x, dh, dw))
    plain = actx.resize_cubic_f32(x, dw, dh)
    assert not np.array_equal(got[:, 0], plain[:, 0]) and not np.array_equal(got[:, -1], plain[:, -1]), "the border columns differ"
    err = np.abs(got.astype(np.float64) - R.torch64(x, dh, dw)).max()
    print(f"x2: |got - torch float64 antialiased| = {err:.3g}")
    assert err <= R.TOL * float(np.abs(x).max())


def test_the_same_size_returns_the_input(actx):
    x = plane(5, 7, 9)
    assert np.array_equal(aa_plane(actx, x, 5, 7), x)


# ---- both forms give the same bits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,sw,dh,dw", [SMALL[0], RATIO4[1]], ids=lambda v: str(v))
def test_both_forms_give_the_same_bits(tctx, sh, sw, dh, dw):
    lib = hooks()
    x = torch.from_numpy(np.stack([plane(sh, sw, 7), plane(sh, sw, 8)])[None]).cuda()
    lib.srcnn_debug_resample_aa_form(-1)
    a = aa_dev(tctx, x, dh, dw)
    assert lib.srcnn_debug_resample_aa_last_form() == 1, "the tiled form where the choice is the library's"
    lib.srcnn_debug_resample_aa_form(0)
    b = aa_dev(tctx, x, dh, dw)
    assert lib.srcnn_debug_resample_aa_last_form() == 0, "the general form through the hook"
    assert same_bits(a, b)
    assert same_bits(a[0, 1], model(x[0, 1].cpu().numpy(), dh, dw))


# ---- layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,sw,dh,dw", [(46, 77, 23, 35), (45, 130, 9, 13)], ids=lambda v: str(v))
def test_padded_strides_and_pitches_in_guarded_buffers(actx, sh, sw, dh, dw):
    """3 channels x 2 frames, row strides, channel pitches and frame pitches padded on both sides; the destination is a window
    of a guard-filled buffer that starts one element off its base (no row of it is 16-byte aligned in step with the others)."""
    n, c = 2, 3
    x = torch.from_numpy(R.uniform((n, c, sh, sw), 31))
    want = aa_dev(actx, x.cuda(), dh, dw)
    src_parent = torch.full((n, c + 1, sh + 5, sw + 7), GUARD)
    src_parent[:, :c, 2:2 + sh, 3:3 + sw] = x
    src_parent = src_parent.cuda()
    src = src_parent[:, :c, 2:2 + sh, 3:3 + sw]
    stride, ch, frame = dw + 5, (dh + 1) * (dw + 5) + 3, c * ((dh + 1) * (dw + 5) + 3) + 11
    dst_parent = torch.full((1 + n * frame + 8,), GUARD, device="cuda")
    dst = dst_parent.as_strided((n, c, dh, dw), (frame, ch, stride, 1), 1)
    torch.cuda.synchronize()
    actx.resize_cubic_aa_f32_dev(src.data_ptr(), src.stride(2), src.stride(1), src.stride(0), sw, sh,
                                 dst.data_ptr(), stride, ch, frame, dw, dh, c, n)
    actx.synchronize()
    assert same_bits(dst.contiguous(), want)
    for f in range(n):
        for k in range(c):
            assert same_bits(want[f, k], model(x[f, k].numpy(), dh, dw)), (f, k)
    outside = torch.ones_like(dst_parent, dtype=torch.bool)
    outside.as_strided((n, c, dh, dw), (frame, ch, stride, 1), 1).fill_(False)
    assert torch.isnan(dst_parent[outside]).all(), "every guard element around the destination is intact"


def test_host_form_equals_device_form(actx):
    sh, sw, dh, dw = 46, 77, 23, 35
    x = R.uniform((3, sh, sw), 41)
    want = aa_dev(actx, torch.from_numpy(x)[None].cuda(), dh, dw)[0].cpu().numpy()
    assert same_bits(actx.resize_cubic_aa_f32(x, dw, dh), want)
    assert same_bits(actx.resize_cubic_aa_f32(x[1], dw, dh), want[1])
    wide = np.full((3, sh + 2, sw + 5), np.float32(GUARD))
    wide[:, 1:1 + sh, 2:2 + sw] = x
    assert same_bits(actx.resize_cubic_aa_f32(wide[:, 1:1 + sh, 2:2 + sw], dw, dh), want)


# ---- stored formats: store(f32 call(load(x))) ---------------------------------------------------------------------------------
BY_NAME = {f[0]: f for f in IR.FORMATS}
PAIRS = [("interleaved-u8", "interleaved-u8"), ("interleaved-f16", "planar-f32"), ("planar-bf16", "interleaved-u8"), ("rgba-u8", "rgba-u8")]


def stored_source(elem, shape, seed):
    rng = np.random.default_rng(seed)
    if elem == IR.U8:
        return rng.integers(0, 256, shape).astype(np.uint8), 1.0 / 255.0
    return IR.store(rng.random(shape, dtype=np.float32), elem), 1.0


@pytest.mark.parametrize("sname,dname", PAIRS)
@pytest.mark.parametrize("sh,sw,dh,dw", [(46, 77, 23, 35), (45, 130, 9, 13)], ids=lambda v: str(v))
def test_stored_formats(actx, sh, sw, dh, dw, sname, dname):
    """The second geometry runs the general form.  rgba-u8 has px_step 4 on both sides: the destination's alpha bytes lie
    outside the image and are guards like the padding."""
    sfmt, dfmt = BY_NAME[sname], BY_NAME[dname]
    src_bits, sscale = stored_source(sfmt[1], (1, 3, sh, sw), sh + len(sname))
    ref = aa_dev(actx, torch.from_numpy(IR.load(src_bits, sfmt[1], sscale)).cuda(), dh, dw).cpu().numpy()
    s = Buf(sfmt, 1, 3, sh, sw, sscale, off=1, row_pad=3).put(src_bits)
    d = Buf(dfmt, 1, 3, dh, dw, 255.0, off=1, row_pad=5)
    run(actx.resize_cubic_aa_image_dev, s.image, sw, sh, d.image, dw, dh, 3, 1)
    want = IR.store(ref, d.elem, 255.0)
    assert IR.same_stored(d.get(), want, d.elem)
    assert d.guards_intact() and s.guards_intact()
    if d.elem == IR.U8:
        assert len(np.unique(want)) > 16


def test_three_frames_against_three_calls(actx):
    sh, sw, dh, dw = 46, 77, 23, 35
    fmt = BY_NAME["interleaved-u8"]
    src_bits, scale = stored_source(IR.U8, (3, 3, sh, sw), 77)
    s = Buf(fmt, 3, 3, sh, sw, scale, frame_pad=7).put(src_bits)
    d = Buf(fmt, 3, 3, dh, dw, 255.0, frame_pad=5)
    run(actx.resize_cubic_aa_image_dev, s.image, sw, sh, d.image, dw, dh, 3, 3)
    one = Buf(fmt, 1, 3, dh, dw, 255.0)
    for f in range(3):
        run(actx.resize_cubic_aa_image_dev, s.frame(f), sw, sh, one.image, dw, dh, 3, 1)
        assert np.array_equal(d.get()[f], one.get()[0]), f
    assert d.guards_intact()


# ---- torch -------------------------------------------------------------------------------------------------------------------
def test_torch_methods_on_both_kinds_of_stream():
    fast = compile_module(make_module(3, 1, "zeros", 6), input_range=2.0)
    try:
        sh, sw, dh, dw = 46, 77, 23, 35
        x = torch.from_numpy(R.uniform((2, 3, sh, sw), 71)).cuda()
        u8 = (x * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # N x H x W x 3 bytes
        want = aa_dev(fast.ctx, x, dh, dw)
        plain = fast.resize(x, (dh, dw))
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            r = fast.resize(x, (dh, dw), antialias=True)
            z = r * 2.0 + 1.0                          # the next torch op on that stream consumes the result unsynchronised
            img = fast.resize_image(u8, (dh, dw), antialias=True)
        stream.synchronize()
        assert same_bits(r, want) and same_bits(z, want * 2.0 + 1.0)
        rd = fast.resize(x * 1.0, (dh, dw), antialias=True)          # the default stream, behind torch's own work on it
        imgd = fast.resize_image(u8.clone(memory_format=torch.preserve_format), (dh, dw), antialias=True)
        torch.cuda.synchronize()
        assert same_bits(rd, want) and torch.equal(imgd, img)
        # the image method against the Context call on the same descriptors
        assert img.dtype == torch.uint8 and img.shape == (2, 3, dh, dw) and img.permute(0, 2, 3, 1).is_contiguous()
        out = torch.zeros((2, dh, dw, 3), dtype=torch.uint8, device="cuda")
        src = S.Image(u8.data_ptr(), S.ELEM_U8, 3, sw * 3, 1, sh * sw * 3, 1.0 / 255.0)
        dst = S.Image(out.data_ptr(), S.ELEM_U8, 3, dw * 3, 1, dh * dw * 3, 255.0)
        run(fast.ctx.resize_cubic_aa_image_dev, src, sw, sh, dst, dw, dh, 3, 2)
        assert torch.equal(img.permute(0, 2, 3, 1), out)
        # torch's own antialiased resize, in float64 on the CPU
        ref = R.torch64(x.cpu().numpy(), dh, dw)
        err = np.abs(r.cpu().numpy().astype(np.float64) - ref).max()
        print(f"|resize(antialias=True) - F.interpolate float64| = {err:.3g}")
        assert err <= R.TOL * float(x.abs().max())
        # antialias=False is today's resize
        assert same_bits(fast.resize(x, (dh, dw), antialias=False), plain) and not same_bits(plain, want)
        assert torch.equal(fast.resize_image(u8, (dh, dw), antialias=False), fast.resize_image(u8, (dh, dw)))
        with pytest.raises(ValueError, match="antialias"):
            fast.resize(x, (dh, dw), antialias=1)
    finally:
        fast.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_invalid_arguments_leave_the_context_usable(actx):
    sh, sw, dh, dw = 46, 77, 23, 35
    x = torch.from_numpy(R.uniform((1, 2, sh, sw), 91)).cuda()
    want = aa_dev(actx, x, dh, dw)
    out = torch.zeros((1, 2, dh, dw), device="cuda")
    big = torch.zeros(4 * sh * sw, device="cuda")
    torch.cuda.synchronize()
    p, q, sp, dp = x.data_ptr(), out.data_ptr(), sh * sw, dh * dw
    r = actx.resize_cubic_aa_f32_dev
    for bad in (lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, 0, dh, 2, 1),                # size 0
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, -3, 2, 1),
                lambda: r(p, sw, sp, 0, 0, sh, q, dw, dp, 0, dw, dh, 2, 1),
                lambda: r(p, sw - 1, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 2, 1),           # stride below the width
                lambda: r(p, sw, sp, 0, sw, sh, q, dw - 1, dp, 0, dw, dh, 2, 1),
                lambda: r(0, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 2, 1),               # null pointers
                lambda: r(p, sw, sp, 0, sw, sh, 0, dw, dp, 0, dw, dh, 2, 1),
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 0, 1),               # no channels, no frames
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 2, 0),
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp // 2, 0, dw, dh, 2, 1),          # output planes overlap each other
                lambda: r(p, sw, sp, 0, sw, sh, q, dw, dp, 0, dw, dh, 1, 2),               # two frames written to one place
                lambda: r(big.data_ptr(), sw, sp, 0, sw, sh, big.data_ptr() + 4 * sp, dw, dp, 0, dw, dh, 2, 1)):   # output over input
        assert "resize_cubic_aa_f32_dev" in _err(bad, S.ERR_INVALID)
        assert same_bits(aa_dev(actx, x, dh, dw), want), "a successful call on the same context after the refusal"
    with pytest.raises(S.SrcnnError):
        actx._check(actx._lib.srcnn_resize_cubic_aa_f32(actx._h, None, sw, sp, sw, sh, S._fp(np.empty((2, dh, dw), np.float32)), dw, dp,
                                                        dw, dh, 2))
    assert same_bits(actx.resize_cubic_aa_f32(x[0].cpu().numpy(), dw, dh), want[0])
    # descriptors srcnn_image_check refuses, and a destination over the source
    s = Buf(PLANAR_F32, 1, 2, sh, sw).put(IR.store(x.cpu().numpy(), IR.F32))
    d = Buf(PLANAR_F32, 1, 2, dh, dw)
    call = actx.resize_cubic_aa_image_dev
    no_scale = S.Image(d.image.ptr, S.ELEM_U8, 1, dw, dh * dw, 0, 0.0)
    folded = S.Image(d.image.ptr, S.ELEM_F32, 1, dw, dw, 0)                                # channel pitch inside the plane
    over = S.Image(s.image.ptr + 4, S.ELEM_F32, 1, dw, dh * dw, 0)
    for bad in (lambda: call(s.image, sw, sh, no_scale, dw, dh, 2, 1), lambda: call(s.image, sw, sh, folded, dw, dh, 2, 1),
                lambda: call(s.image, sw, sh, over, dw, dh, 2, 1), lambda: call(s.image, sw, 0, d.image, dw, dh, 2, 1)):
        assert "resize_cubic_aa_image_dev" in _err(bad, S.ERR_INVALID)
        run(call, s.image, sw, sh, d.image, dw, dh, 2, 1)
        assert np.array_equal(d.get(), bits(want)), "a successful call on the same context after the refusal"
    assert actx._lib.srcnn_abi_version() == 1
