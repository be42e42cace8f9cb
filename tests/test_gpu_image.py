"""Images as they are stored, on the GPU (srcnn_forward_image_dev, srcnn_resize_cubic_image_dev, srcnn_process_image_dev,
srcnn_process_rgb_image_dev and the torch methods on them).  The rule under test is bitwise: each call equals
store(existing float32 call(load(x))).  Expected values are computed on the host from the downloaded result of the existing
planar-float32 call on load(x), passed through the reference store (tests/image_reference.py, pinned to torch's CPU ops by
tests/test_image_cpu.py).  All images are small."""
import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd import torch_api
import image_reference as R
from color_reference import random_color_model
from resize_f32_reference import TOL
from rgb_f32_reference import BT601_FULL, BT601_STUDIO, classic64, luma_lr_f32
from spatial_reference import random_model, torch_forward
from test_gpu_f32 import reference as model64_planes, scaled_tolerance, unit_planes
from test_gpu_resize_f32 import HEIGHT_CASES, PROCESS_SHAPES
from zero_pad_reference import torch_forward_zero

pytestmark = pytest.mark.gpu

MODES = [S.MODE_MFMA, S.MODE_BANDED16]
LUMAS = [BT601_FULL.luma(), BT601_STUDIO.luma(), S.luma_for_order(S.LUMA_BT601, "bgr")]      # those of tests/test_gpu_rgb_f32.py
CLAMP = (0.0, 1.0)
TORCH_BITS = {R.F32: torch.int32, R.F16: torch.int16, R.BF16: torch.int16, R.U8: torch.uint8}
SIGNED = {R.F32: np.int32, R.F16: np.int16, R.BF16: np.int16, R.U8: np.uint8}
GUARD = {R.F32: 0x7FC00123, R.F16: 0x7E55, R.BF16: 0x7FA5, R.U8: 0xA5}
PLANAR_F32 = R.FORMATS[0]


@pytest.fixture(scope="module")
def ictx():
    ctx = S.Context(0)
    yield ctx
    ctx.close()


def unit_model(channels, f2, seed):
    """A random model for [0, 1] data: the suite's random models are made for 0 .. 255 data (on [0, 1] their output is their
    biases and next to constant), so the biases are divided by 255 -- model_unit(x) = model(255 x) / 255."""
    w1, b1, w2, b2, w3, b3 = random_color_model(f2, seed) if channels == 3 else random_model(f2, seed)
    s = np.float32(1.0 / 255.0)
    return w1, b1 * s, w2, b2 * s, w3, (b3 * s if channels == 3 else float(np.float32(b3) * s))


def load_model(ctx, channels, f2, padding, mode, seed=3):
    ctx.set_model(*unit_model(channels, f2, seed))
    ctx.set_padding(padding)
    ctx.set_mode(mode)
    ctx.set_input_range(2.0)          # [0, 1] data and the overshoot of a resize


class Buf:
    """An image in device memory, held as bits in a guard-filled 1-D tensor: `view` is its logical (n, c, h, w) window."""

    def __init__(self, fmt, n, c, h, w, scale=1.0, off=0, row_pad=0, frame_pad=0):
        _, self.elem, kind = fmt
        px, stride, ch, frame = R.layout(kind, c, h, w, row_pad, frame_pad)
        self.shape, self.strides, self.off = (n, c, h, w), (frame, ch, stride, px), off
        total = off + (n - 1) * frame + (c - 1) * ch + (h - 1) * stride + (w - 1) * px + 1 + 9
        self.parent = torch.full((total,), GUARD[self.elem], dtype=TORCH_BITS[self.elem], device="cuda")
        self.view = self.parent.as_strided(self.shape, self.strides, off)
        self.image = S.Image(self.view.data_ptr(), self.elem, px, stride, ch, frame, scale)

    def put(self, bits):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(bits).view(SIGNED[self.elem])).cuda())
        return self

    def get(self):
        return self.view.contiguous().cpu().numpy().view(R.BITS[self.elem])

    def frame(self, f):
        """Frame f as an image of its own."""
        im = self.image
        return S.Image(self.view[f].data_ptr(), im.elem, im.px_step, im.stride, im.ch_pitch, 0, im.scale)

    def guards_intact(self):
        outside = torch.ones(self.parent.shape, dtype=torch.bool, device="cuda")
        outside.as_strided(self.shape, self.strides, self.off).fill_(False)
        return bool((self.parent[outside] == GUARD[self.elem]).all())


def run(call, *args):
    torch.cuda.synchronize()
    call(*args)
    torch.cuda.synchronize()


def f32_call(ctx, x, out_shape, call):
    """An existing planar-float32 device call on contiguous tensors: x (n, c, h, w) numpy -> numpy of out_shape."""
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    out = torch.full(out_shape, float("nan"), dtype=torch.float32, device="cuda")
    n, c, h, w = x.shape
    _, oc, dh, dw = out_shape
    run(call, (xd.data_ptr(), w, h * w, c * h * w), (out.data_ptr(), dw, dh * dw, oc * dh * dw))
    return out.cpu().numpy()


def shared_sources(shape, seed):
    """The same values in every element kind: x = b / 256 for random bytes b is exact in float16 and bfloat16, and a U8 load
    with scale 1 / 256.  {elem: (bits, scale)} and x."""
    b = np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)
    x = b.astype(np.float32) / np.float32(256)
    src = {R.F32: (R.store(x, R.F32), 1.0), R.F16: (R.store(x, R.F16), 1.0), R.BF16: (R.store(x, R.BF16), 1.0), R.U8: (b, 1.0 / 256.0)}
    for elem, (bits, scale) in src.items():
        assert np.array_equal(R.load(bits, elem, scale), x)
    return src, x


def own_source(elem, shape, seed):
    """Values of the element kind's own: random bytes read with 1 / 255 (a rounded multiply), or [0, 1) rounded to the kind."""
    rng = np.random.default_rng(seed)
    if elem == R.U8:
        return rng.integers(0, 256, shape).astype(np.uint8), 1.0 / 255.0
    return R.store(rng.random(shape, dtype=np.float32), elem), 1.0


def u8_scale_for(ref):
    """A store scale that puts the result's upper decile above 255.5 and the rest below (part of the test's input): the byte
    result then holds saturated and rounded values."""
    return float(np.float32(255.5 / max(float(np.quantile(np.abs(ref[np.isfinite(ref)]), 0.9)), 1e-6)))


def varied(want):
    """A byte result that is not one value: some of it saturated, some not (a single pixel excepted)."""
    return want.size < 8 or (len(np.unique(want)) > 1 and want.min() < 255)


def check_matrix(image_call, f32_ref, n, c, h, w, dh, dw, seed, formats=R.FORMATS, **hard):
    """Every source format against a planar-float32 destination, every destination format against a planar-float32 source,
    and three mixed pairs; image_call(src_image, dst_image), f32_ref(x) -> the existing call's float32 result (n, c, dh, dw)."""
    src, x = shared_sources((n, c, h, w), seed)
    ref = f32_ref(x)
    assert ref.shape == (n, c, dh, dw) and np.isfinite(ref).all()
    oscale = u8_scale_for(ref)

    def one(sfmt, bits, sscale, dfmt, want_ref, what):
        s = Buf(sfmt, n, c, h, w, sscale, **hard).put(bits)
        d = Buf(dfmt, n, c, dh, dw, oscale, **hard)
        run(image_call, s.image, d.image)
        want = R.store(want_ref, d.elem, oscale)
        assert R.same_stored(d.get(), want, d.elem), what
        assert d.guards_intact() and s.guards_intact(), what
        if d.elem == R.U8:
            assert varied(want), "the byte result is not all saturated"

    for fmt in formats:
        one(fmt, *src[fmt[1]], PLANAR_F32, ref, f"{fmt[0]} -> planar-f32")
        one(PLANAR_F32, *src[R.F32], fmt, ref, f"planar-f32 -> {fmt[0]}")
    by_name = {f[0]: f for f in R.FORMATS}
    for sname, dname in (("interleaved-u8", "interleaved-u8"), ("interleaved-f16", "interleaved-f16"), ("planar-bf16", "interleaved-f32")):
        sfmt, dfmt = by_name[sname], by_name[dname]
        bits, sscale = own_source(sfmt[1], (n, c, h, w), seed + 1)
        one(sfmt, bits, sscale, dfmt, f32_ref(R.load(bits, sfmt[1], sscale)), f"{sname} -> {dname}")


def forward_matrix(ctx, channels, w, h, seed, n=1, **kw):
    check_matrix(lambda s, d: ctx.forward_image_dev(s, d, w, h, n),
                 lambda x: f32_call(ctx, x, x.shape, lambda a, b: ctx.forward_f32_dev(*a, *b, w, h, n)),
                 n, channels, h, w, h, w, seed, **kw)


# ---- 6: forward_image, bitwise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("padding", ["replicate", "zero"])
@pytest.mark.parametrize("f2", [1, 5])
@pytest.mark.parametrize("channels", [1, 3])
def test_forward_image_at_130x67(ictx, channels, f2, padding, mode):
    """130 x 67 crosses the 128-column layer-1 tile, the 124-column layer-3 strip and the 8- and 16-row tiles."""
    load_model(ictx, channels, f2, padding, mode)
    forward_matrix(ictx, channels, 130, 67, 10 * f2 + channels)


@pytest.mark.parametrize("w,h", [(1, 1), (9, 5), (260, 75)])
@pytest.mark.parametrize("channels,f2,padding", [(3, 5, "zero"), (1, 1, "replicate")])
def test_forward_image_at_the_other_sizes(ictx, channels, f2, padding, w, h):
    load_model(ictx, channels, f2, padding, S.MODE_MFMA)
    forward_matrix(ictx, channels, w, h, w + channels)


# ---- 7: resize_cubic_image, bitwise ----------------------------------------------------------------------------------------
RESIZE_CASES = HEIGHT_CASES + [(40, 131, 80, 262), (23, 29, 11, 13)]      # tile bounds, x2 across column 256, the direct form


def resize_ref(ctx, c, sw, sh, dw, dh, n=1):
    return lambda x: f32_call(ctx, x, (n, c, dh, dw), lambda a, b: ctx.resize_cubic_f32_dev(*a, sw, sh, *b, dw, dh, c, n))


@pytest.mark.parametrize("sh,sw,dh,dw", RESIZE_CASES, ids=lambda v: str(v))
def test_resize_image(ictx, sh, sw, dh, dw):
    import ctypes as C
    tuning = C.CDLL(str(S.tuning_library_path()))
    tuning.srcnn_debug_resize_f32_variant.argtypes = [C.c_int] * 4
    assert tuning.srcnn_debug_resize_f32_variant(sw, sh, dw, dh) == (0 if (sh, sw) == (23, 29) else 1), "the form the case is for"
    check_matrix(lambda s, d: ictx.resize_cubic_image_dev(s, sw, sh, d, dw, dh, 3, 1), resize_ref(ictx, 3, sw, sh, dw, dh),
                 1, 3, sh, sw, dh, dw, sh + dw)


def test_same_size_resize_is_a_format_conversion(ictx):
    """The store's ties, overflow and NaN on the GPU: a same-size call on the special values, each isolated in a plane of
    zeros far enough from the next (the four taps of a same-size resize are {0, 1, 0, 0}: a non-finite value would turn its
    neighbours into NaN, which the rule allows and the expectation, computed from the existing call, contains)."""
    special = np.array([0.5, 1.5, 2.5, 254.5, 255.0, 255.5, 256.0, -0.5, -3.0, 1e9, 65504.0, 65519.9, 65520.0, -65520.0, 2.0 ** -24,
                        2.0 ** -25, 1.5 * 2.0 ** -24, 1e-40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 3.3895314e38,
                        np.inf, -np.inf, np.nan, 0.49999997, 127.5, 128.5], dtype=np.float32)
    h, w = 9, 8 * len(special)
    x = np.zeros((1, 1, h, w), np.float32)
    x[0, 0, 4, 4::8] = special
    ref = resize_ref(ictx, 1, w, h, w, h)(x)
    assert R.same_stored(ref.view(np.uint32)[0, 0, 4, 4::8], special.view(np.uint32), R.F32), "an exact copy of the values themselves"
    s = Buf(PLANAR_F32, 1, 1, h, w).put(R.store(x, R.F32))
    for fmt in R.FORMATS:
        for off in (0, 1):
            d = Buf(fmt, 1, 1, h, w, 1.0, off=off)
            run(ictx.resize_cubic_image_dev, s.image, w, h, d.image, w, h, 1, 1)
            want = R.store(ref, d.elem, 1.0)
            assert R.same_stored(d.get(), want, d.elem) and d.guards_intact(), (fmt[0], off)
    u8 = R.store(ref, R.U8, 1.0)[0, 0, 4, 4::8]
    assert list(u8[:10]) == [0, 2, 2, 254, 255, 255, 255, 0, 0, 255] and u8[24] == 0 and list(u8[25:]) == [0, 128, 128]
    # and the loads: every byte, every float16 and bfloat16 bit pattern of a sample, converted to float32
    for fmt, bits, scale in ((R.FORMATS[4], np.arange(256, dtype=np.uint8), 1.0 / 255.0),
                             (R.FORMATS[2], np.arange(0, 1 << 16, 7, dtype=np.uint16), 1.0),
                             (R.FORMATS[3], np.arange(0, 1 << 16, 7, dtype=np.uint16), 1.0)):
        finite = np.isfinite(R.load(bits, fmt[1], scale))
        bits = bits[finite][: (finite.sum() // 16) * 16].reshape(1, 1, 16, -1)
        wv = bits.shape[3]
        sb = Buf(fmt, 1, 1, 16, wv, scale).put(bits)
        d = Buf(PLANAR_F32, 1, 1, 16, wv)
        run(ictx.resize_cubic_image_dev, sb.image, wv, 16, d.image, wv, 16, 1, 1)
        xl = R.load(bits, fmt[1], scale)
        assert R.same_stored(d.get(), R.store(resize_ref(ictx, 1, wv, 16, wv, 16)(xl), R.F32), R.F32), fmt[0]
        assert np.array_equal(np.abs(d.get().view(np.float32)), np.abs(xl)), "the load itself (a zero's sign apart: 0 * s0 + 1 * s1)"


# ---- 8: process_image and process_rgb_image --------------------------------------------------------------------------------
PROCESS_CASES = PROCESS_SHAPES + [(40, 131, 80, 262)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("channels,f2,padding", [(3, 5, "zero"), (1, 1, "replicate")])
@pytest.mark.parametrize("sh,sw,dh,dw", PROCESS_CASES, ids=lambda v: str(v))
def test_process_image(ictx, sh, sw, dh, dw, channels, f2, padding, mode):
    load_model(ictx, channels, f2, padding, mode)
    check_matrix(lambda s, d: ictx.process_image_dev(s, sw, sh, d, dw, dh, 1),
                 lambda x: f32_call(ictx, x, (1, channels, dh, dw), lambda a, b: ictx.process_f32_dev(*a, sw, sh, *b, dw, dh, 1)),
                 1, channels, sh, sw, dh, dw, sh + f2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f2,padding", [(5, "zero"), (1, "replicate")])
@pytest.mark.parametrize("case", list(enumerate(PROCESS_CASES)), ids=lambda c: str(c[1]))
def test_process_rgb_image(ictx, case, f2, padding, mode):
    k, (sh, sw, dh, dw) = case
    load_model(ictx, 1, f2, padding, mode)
    for j, clamp in enumerate((None, CLAMP)):
        luma = LUMAS[(k + j + f2) % 3]
        check_matrix(lambda s, d: ictx.process_rgb_image_dev(s, sw, sh, d, dw, dh, luma, clamp, 1),
                     lambda x: f32_call(ictx, x, (1, 3, dh, dw),
                                        lambda a, b: ictx.process_rgb_f32_dev(*a, sw, sh, *b, dw, dh, luma, clamp, 1)),
                     1, 3, sh, sw, dh, dw, sh + f2 + j)


# ---- 9: layout hardening ---------------------------------------------------------------------------------------------------
HARD = dict(off=1, row_pad=5, frame_pad=7)      # an odd u8 address, 2 mod 4 for the 16-bit kinds; padded rows and frames


def test_hardened_layouts_and_three_frames(ictx):
    """Guard-filled buffers whose base is one element off, padded rows, three frames with a padded frame pitch: the guards and
    the alpha bytes of an RGBA destination stay untouched (Buf.guards_intact inside check_matrix), and three frames equal three
    single calls."""
    n, sh, sw, dh, dw = 3, 20, 24, 40, 48
    load_model(ictx, 3, 1, "zero", S.MODE_MFMA)
    forward_matrix(ictx, 3, 70, 19, 77, n=n, **HARD)
    check_matrix(lambda s, d: ictx.resize_cubic_image_dev(s, sw, sh, d, dw, dh, 3, n), resize_ref(ictx, 3, sw, sh, dw, dh, n),
                 n, 3, sh, sw, dh, dw, 78, **HARD)
    check_matrix(lambda s, d: ictx.process_image_dev(s, sw, sh, d, dw, dh, n),
                 lambda x: f32_call(ictx, x, (n, 3, dh, dw), lambda a, b: ictx.process_f32_dev(*a, sw, sh, *b, dw, dh, n)),
                 n, 3, sh, sw, dh, dw, 79, **HARD)
    load_model(ictx, 1, 5, "replicate", S.MODE_BANDED16)
    check_matrix(lambda s, d: ictx.process_rgb_image_dev(s, sw, sh, d, dw, dh, LUMAS[0], CLAMP, n),
                 lambda x: f32_call(ictx, x, (n, 3, dh, dw),
                                    lambda a, b: ictx.process_rgb_f32_dev(*a, sw, sh, *b, dw, dh, LUMAS[0], CLAMP, n)),
                 n, 3, sh, sw, dh, dw, 80, **HARD)
    # three frames in one call equal three single calls, frame by frame, in a stored format on both sides
    fmt = R.FORMATS[5]                                      # RGBA u8
    bits, scale = own_source(R.U8, (n, 3, sh, sw), 81)
    s = Buf(fmt, n, 3, sh, sw, scale, **HARD).put(bits)
    calls = {"resize": lambda a, b, k: ictx.resize_cubic_image_dev(a, sw, sh, b, dw, dh, 3, k),
             "process_rgb": lambda a, b, k: ictx.process_rgb_image_dev(a, sw, sh, b, dw, dh, LUMAS[1], None, k)}
    for name, call in calls.items():
        many, single = Buf(fmt, n, 3, dh, dw, 255.0, **HARD), Buf(fmt, n, 3, dh, dw, 255.0, **HARD)
        run(call, s.image, many.image, n)
        for f in range(n):
            run(call, s.frame(f), single.frame(f), 1)
        assert np.array_equal(many.get(), single.get()) and many.guards_intact() and single.guards_intact(), name
        assert varied(many.get())


def rows_interleaved_f32(h, w, off=1):
    """A planar float32 image of three channels interleaved by ROW (stride 3 w, channel pitch w): a layout srcnn_image_check
    accepts and the gate of the _f32_dev calls refuses, a channel pitch inside the row stride."""
    b = Buf.__new__(Buf)
    b.elem, b.shape, b.strides, b.off = R.F32, (1, 3, h, w), (3 * h * w, w, 3 * w, 1), off
    b.parent = torch.full((off + 3 * h * w + 9,), GUARD[R.F32], dtype=TORCH_BITS[R.F32], device="cuda")
    b.view = b.parent.as_strided(b.shape, b.strides, off)
    b.image = S.Image(b.view.data_ptr(), R.F32, 1, 3 * w, w, 3 * h * w, 1.0)
    return b


def test_planar_float32_the_float_gate_refuses_equals_packed_planes(ictx):
    """Planar float32 on both sides in a layout the _f32_dev gate refuses: resize_cubic_image_dev, process_rgb_image_dev (front
    and merge) and process_image_dev (the resize into the workspace) on a destination whose channels are interleaved by row.
    Each equals the same call on packed planes bit for bit, in guard-filled buffers one element off their base; 131 x 40 ->
    262 x 80 is the tiled form with a ragged right edge and three row tiles, 40 x 30 -> 20 x 15 the direct form.  What this
    pins is the addressing of such a layout (strides, pitches, the stores' alignment rule); which kernel a launch takes is the
    launchers' rule (both sides planar float32: the float32 one) and is not observed here, and the arithmetic of either
    kernel is what the other tests of this file and tests/test_gpu_resize_f32.py pin."""
    def same_as_packed(call, sh, sw, dh, dw, seed):
        bits = R.store(np.random.default_rng(seed).random((1, 3, sh, sw), dtype=np.float32), R.F32)
        s = Buf(PLANAR_F32, 1, 3, sh, sw, off=1).put(bits)
        packed, rows = Buf(PLANAR_F32, 1, 3, dh, dw, off=1), rows_interleaved_f32(dh, dw)
        assert S.image_check(rows.image, dw, dh, 3, 1, True)
        for d in (packed, rows):
            run(call, s.image, d.image)
            assert d.guards_intact() and s.guards_intact()
        want = packed.get()
        assert np.isfinite(want.view(np.float32)).all() and len(np.unique(want)) > dh, "written, and not one value"
        assert np.array_equal(rows.get(), want)

    import ctypes as C
    tuning = C.CDLL(str(S.tuning_library_path()))
    tuning.srcnn_debug_resize_f32_variant.argtypes = [C.c_int] * 4
    assert tuning.srcnn_debug_resize_f32_variant(131, 40, 262, 80) == 1 and tuning.srcnn_debug_resize_f32_variant(40, 30, 20, 15) == 0
    same_as_packed(lambda s, d: ictx.resize_cubic_image_dev(s, 131, 40, d, 262, 80, 3, 1), 40, 131, 80, 262, 91)
    same_as_packed(lambda s, d: ictx.resize_cubic_image_dev(s, 40, 30, d, 20, 15, 3, 1), 30, 40, 15, 20, 92)
    load_model(ictx, 1, 5, "replicate", S.MODE_BANDED16)
    for j, clamp in enumerate((None, CLAMP)):
        same_as_packed(lambda s, d: ictx.process_rgb_image_dev(s, 131, 40, d, 262, 80, LUMAS[j], clamp, 1), 40, 131, 80, 262, 93 + j)
    load_model(ictx, 3, 5, "zero", S.MODE_MFMA)
    same_as_packed(lambda s, d: ictx.process_image_dev(s, 131, 40, d, 262, 80, 1), 40, 131, 80, 262, 95)


# ---- 10: against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f2,padding,mode", [(1, "replicate", S.MODE_MFMA), (5, "zero", S.MODE_BANDED16)])
def test_upscale_rgb_image_against_the_classic_script_in_float64(f2, padding, mode):
    """An H x W x 3 uint8 picture through upscale_rgb_image, against the script it replaces in float64: bytes / 255, resize,
    the full Y'CbCr matrix, the model on Y (on the GPU's own Yup, as tests/test_gpu_rgb_f32.py does, so that only the model's
    arithmetic error enters), the exact inverse, times 255, clamp to [0, 255], round.  Bound per pixel: 0.5 for the store's
    rounding plus 255 times that suite's tolerance `tol`; the clamp to [0, 255] is 1-Lipschitz and adds nothing, so no pixel
    is left out."""
    sh, sw, dh, dw = 30, 61, 60, 122
    model = unit_model(1, f2, 3)
    model64 = (lambda y: torch_forward(y, model)) if padding == "replicate" else (lambda y: torch_forward_zero(y, model))
    ctx = S.Context(0)
    fast = torch_api.CompiledModule(ctx, 1, 0)
    try:
        load_model(ctx, 1, f2, padding, mode)
        hwc = np.random.default_rng(11).integers(0, 256, (sh, sw, 3)).astype(np.uint8)
        x = R.load(np.ascontiguousarray(np.moveaxis(hwc, 2, 0)), R.U8, 1.0 / 255.0)
        conv, luma = BT601_FULL, BT601_FULL.luma()
        got = fast.upscale_rgb_image(torch.from_numpy(hwc).cuda().permute(2, 0, 1), scale=2, luma=luma)
        assert got.dtype == torch.uint8 and got.shape == (3, dh, dw) and got.stride() == (1, dw * 3, 3)
        yup = f32_call(ctx, luma_lr_f32(x, luma)[None, None], (1, 1, dh, dw),
                       lambda a, b: ctx.resize_cubic_f32_dev(*a, sw, sh, *b, dw, dh, 1, 1))[0, 0]
        ref = classic64(x, dh, dw, conv, model64, yup=yup)
        g = S.luma_gain(luma)
        tol = g * scaled_tolerance(model64(yup.astype(np.float64)), 1.0) + 2 * TOL * (float(np.abs(x).max()) + g * float(np.abs(yup).max()))
        err = np.abs(got.cpu().numpy().astype(np.float64) - np.clip(ref * 255.0, 0.0, 255.0))
        print(f"9-{f2}-5 {padding} mode {mode}: max |got - clip(ref * 255)| = {err.max():.4f}, bound {0.5 + 255 * tol:.4f}")
        assert (err <= 0.5 + 255.0 * tol).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("channels,f2,padding,mode", [(1, 1, "replicate", S.MODE_MFMA), (3, 5, "zero", S.MODE_BANDED16)])
def test_forward_image_half_outputs_against_float64(ictx, channels, f2, padding, mode):
    """float16 and bfloat16 outputs: the existing tolerance of the float path plus half an ulp of the output format at the
    value (taken at |ref| + tol, which is no smaller than at the stored value's own binade)."""
    w, h = 130, 67
    model = unit_model(channels, f2, 1)
    ictx.set_model(*model)
    ictx.set_padding(padding)
    ictx.set_mode(mode)
    ictx.set_input_range(1.0)
    x = unit_planes(channels, w, h)
    ref = model64_planes(x, model, padding)
    tol = scaled_tolerance(ref, 1.0)
    s = Buf(PLANAR_F32, 1, channels, h, w).put(R.store(x[None], R.F32))
    for fmt in (R.FORMATS[2], R.FORMATS[3]):
        d = Buf(fmt, 1, channels, h, w)
        run(ictx.forward_image_dev, s.image, d.image, w, h, 1)
        got = R.load(d.get(), d.elem)[0].astype(np.float64)
        err = np.abs(got - ref)
        bound = tol + R.half_ulp(np.abs(ref) + tol, d.elem)
        print(f"{fmt[0]}: max error {err.max():.3g}, tolerance {tol:.3g} + half an ulp up to {R.half_ulp(np.abs(ref).max(), d.elem):.3g}")
        assert (err <= bound).all()


# ---- 11: the torch methods -------------------------------------------------------------------------------------------------
def tensor_bits(t):
    return t.contiguous().view(TORCH_BITS[torch_api._elem_of(t.dtype)]).cpu().numpy()


@pytest.mark.parametrize("side_stream", [False, True])
def test_torch_methods_read_where_the_tensor_lies_and_equal_the_context_calls(side_stream):
    sh, sw, dh, dw = 20, 24, 40, 48
    luma_ctx, colour_ctx = S.Context(0), S.Context(0)
    try:
        load_model(luma_ctx, 1, 1, "zero", S.MODE_MFMA)
        load_model(colour_ctx, 3, 5, "replicate", S.MODE_MFMA)
        luma_fast, colour_fast = torch_api.CompiledModule(luma_ctx, 1, 0), torch_api.CompiledModule(colour_ctx, 3, 0)
        rng = np.random.default_rng(21)
        stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
        nhwc = torch.from_numpy(rng.integers(0, 256, (2, sh, sw, 3)).astype(np.uint8)).cuda()        # a batch of 2, H x W x C
        half = torch.from_numpy(rng.random((2, 3, sh, sw), dtype=np.float32)).cuda().half().to(memory_format=torch.channels_last)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            x = nhwc.permute(0, 3, 1, 2)
            out_rgb = luma_fast.upscale_rgb_image(x, scale=2, clamp=CLAMP)
            out_up = colour_fast.upscale_image(half, size=(dh, dw))
            out_fwd = colour_fast.forward_image(half, out_dtype=torch.bfloat16, out_channels_last=False)
            out_res = colour_fast.resize_image(x, (dh, dw), out_dtype=torch.float32, out_channels_last=False)
            out_u8 = colour_fast.forward_image(half[0], out_dtype=torch.uint8, out_scale=100.0)
        torch.cuda.synchronize()
        assert out_rgb.dtype == torch.uint8 and out_rgb.shape == (2, 3, dh, dw) and out_rgb.stride() == (dh * dw * 3, 1, dw * 3, 3)
        assert out_up.dtype == torch.float16 and out_up.shape == (2, 3, dh, dw) and out_up.is_contiguous(memory_format=torch.channels_last)
        assert out_fwd.dtype == torch.bfloat16 and out_fwd.is_contiguous() and out_fwd.shape == (2, 3, sh, sw)
        assert out_res.dtype == torch.float32 and out_res.is_contiguous() and out_res.shape == (2, 3, dh, dw)
        assert out_u8.dtype == torch.uint8 and out_u8.shape == (3, sh, sw) and out_u8.stride() == (1, sw * 3, 3)
        # the same calls on the Context, from descriptors written out by hand, into buffers of the test's own
        u8_in = S.Image(nhwc.data_ptr(), S.ELEM_U8, 3, sw * 3, 1, sh * sw * 3, 1.0 / 255.0)
        f16_in = S.Image(half.data_ptr(), S.ELEM_F16, 3, sw * 3, 1, sh * sw * 3)
        for ctx in (luma_ctx, colour_ctx):
            ctx.set_stream(0)
        d = Buf(R.FORMATS[4], 2, 3, dh, dw, 255.0)
        run(luma_ctx.process_rgb_image_dev, u8_in, sw, sh, d.image, dw, dh, S.LUMA_BT601, CLAMP, 2)
        assert np.array_equal(tensor_bits(out_rgb), d.get()) and varied(d.get())
        d = Buf(R.FORMATS[2], 2, 3, dh, dw)
        run(colour_ctx.process_image_dev, f16_in, sw, sh, d.image, dw, dh, 2)
        assert R.same_stored(tensor_bits(out_up).view(np.uint16), d.get(), R.F16)
        d = Buf(R.FORMATS[3], 2, 3, sh, sw)
        run(colour_ctx.forward_image_dev, f16_in, d.image, sw, sh, 2)
        assert R.same_stored(tensor_bits(out_fwd).view(np.uint16), d.get(), R.BF16)
        d = Buf(PLANAR_F32, 2, 3, dh, dw)
        run(colour_ctx.resize_cubic_image_dev, u8_in, sw, sh, d.image, dw, dh, 3, 2)
        assert R.same_stored(tensor_bits(out_res).view(np.uint32), d.get(), R.F32)
        d = Buf(R.FORMATS[4], 1, 3, sh, sw, 100.0)
        run(colour_ctx.forward_image_dev, S.Image(half.data_ptr(), S.ELEM_F16, 3, sw * 3, 1, 0), d.image, sw, sh, 1)
        assert np.array_equal(tensor_bits(out_u8), d.get()[0])
    finally:
        luma_ctx.close()
        colour_ctx.close()


# ---- 12: refusals ----------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(S.SrcnnError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusals_leave_the_context_usable(weights_blob):
    sh, sw, dh, dw = 20, 24, 40, 48
    fmt = R.FORMATS[4]
    bits, scale = own_source(R.U8, (1, 3, sh, sw), 31)
    with S.Context(0) as ctx:
        s = Buf(fmt, 1, 3, sh, sw, scale).put(bits)
        d = Buf(fmt, 1, 3, dh, dw, 255.0)
        s1 = Buf(fmt, 1, 1, sh, sw, scale).put(bits[:, :1])
        d1 = Buf(fmt, 1, 1, dh, dw, 255.0)
        resize = lambda a=s.image, b=d.image: run(ctx.resize_cubic_image_dev, a, sw, sh, b, dw, dh, 3, 1)
        resize()
        want = d.get().copy()
        assert varied(want)

        def still_good():
            d.parent.fill_(GUARD[R.U8])
            resize()
            assert np.array_equal(d.get(), want) and d.guards_intact()

        def variant(im, **kw):
            v = S.Image(im.ptr, im.elem, im.px_step, im.stride, im.ch_pitch, im.frame_pitch, im.scale)
            for k, val in kw.items():
                setattr(v, k, val)
            return v
        # STATE: no model; the resize needs none
        _err(lambda: ctx.forward_image_dev(s.image, Buf(fmt, 1, 3, sh, sw, 255.0).image, sw, sh, 1), S.ERR_STATE)
        _err(lambda: ctx.process_image_dev(s.image, sw, sh, d.image, dw, dh, 1), S.ERR_STATE)
        _err(lambda: ctx.process_rgb_image_dev(s.image, sw, sh, d.image, dw, dh), S.ERR_STATE)
        still_good()
        # STATE: layers loaded per filter
        from srcnn_cpp_amd.synth import synth_luma
        w1, b1, w2, b2, w3, b3 = S.split_weights(weights_blob)
        y = synth_luma(96, 40)
        planes = [np.empty(y.shape, np.float32) for _ in range(32)]
        ctx.conv99x11(y, planes, w1, b1, w2, b2)
        ctx.conv55(planes, np.empty_like(y), w3, b3)
        for call in (lambda: ctx.process_image_dev(s1.image, sw, sh, d1.image, dw, dh, 1),
                     lambda: ctx.process_rgb_image_dev(s.image, sw, sh, d.image, dw, dh),
                     lambda: ctx.forward_image_dev(s1.image, Buf(fmt, 1, 1, sh, sw, 255.0).image, sw, sh, 1)):
            assert "per-filter" in _err(call, S.ERR_STATE)
        still_good()
        # a whole 1-channel model: the calls run; then a mode without a float path
        ctx.set_weights_blob(weights_blob)
        ctx.set_input_range(2.0)
        run(ctx.process_rgb_image_dev, s.image, sw, sh, d.image, dw, dh)
        want_rgb = d.get().copy()
        for mode in (S.MODE_EXACT, S.MODE_SPLIT16, S.MODE_REFBYTES):
            ctx.set_mode(mode)
            assert f"mode {mode}" in _err(lambda: ctx.process_rgb_image_dev(s.image, sw, sh, d.image, dw, dh), S.ERR_STATE)
            _err(lambda: ctx.process_image_dev(s1.image, sw, sh, d1.image, dw, dh, 1), S.ERR_STATE)
            _err(lambda: ctx.forward_image_dev(s1.image, Buf(fmt, 1, 1, sh, sw, 255.0).image, sw, sh, 1), S.ERR_STATE)
        still_good()
        ctx.set_mode(S.MODE_MFMA)
        # INVALID: descriptors, through every call that takes them; after EACH refusal the good call gives its result again
        bad_sources = [variant(s.image, ptr=0), variant(s.image, elem=7), variant(s.image, scale=0.0), variant(s.image, scale=float("nan")),
                       variant(s.image, px_step=0), variant(s.image, stride=0), variant(s.image, ch_pitch=0),
                       variant(s.image, elem=S.ELEM_F16, ptr=s.image.ptr + 1)]
        bad_dests = [variant(d.image, ptr=0), variant(d.image, elem=-1), variant(d.image, scale=float("inf")),
                     variant(d.image, stride=d.image.stride - 1), variant(d.image, ch_pitch=3), variant(d.image, px_step=2),
                     variant(d.image, ptr=s.image.ptr), variant(d.image, ptr=s.image.ptr + 3 * sw * sh - 1)]      # on the source
        for bad in bad_sources:
            _err(lambda: ctx.resize_cubic_image_dev(bad, sw, sh, d.image, dw, dh, 3, 1), S.ERR_INVALID)
            still_good()
            _err(lambda: ctx.process_rgb_image_dev(bad, sw, sh, d.image, dw, dh), S.ERR_INVALID)
            still_good()
        for bad in bad_dests:
            _err(lambda: ctx.resize_cubic_image_dev(s.image, sw, sh, bad, dw, dh, 3, 1), S.ERR_INVALID)
            still_good()
            _err(lambda: ctx.process_rgb_image_dev(s.image, sw, sh, bad, dw, dh), S.ERR_INVALID)
            still_good()
        # ... and forward_image / process_image, which take the loaded model's channel count (1): their own good call
        f1 = Buf(fmt, 1, 1, sh, sw, 255.0)
        run(ctx.forward_image_dev, s1.image, f1.image, sw, sh, 1)
        run(ctx.process_image_dev, s1.image, sw, sh, d1.image, dw, dh, 1)
        want_f1, want_d1 = f1.get().copy(), d1.get().copy()

        def model_calls_still_good():
            f1.parent.fill_(GUARD[R.U8])
            d1.parent.fill_(GUARD[R.U8])
            run(ctx.forward_image_dev, s1.image, f1.image, sw, sh, 1)
            run(ctx.process_image_dev, s1.image, sw, sh, d1.image, dw, dh, 1)
            assert np.array_equal(f1.get(), want_f1) and np.array_equal(d1.get(), want_d1) and f1.guards_intact() and d1.guards_intact()
        bad_s1 = [variant(s1.image, ptr=0), variant(s1.image, elem=7), variant(s1.image, scale=0.0), variant(s1.image, px_step=0),
                  variant(s1.image, stride=0), variant(s1.image, elem=S.ELEM_F16, ptr=s1.image.ptr + 1)]
        for bad in bad_s1:
            _err(lambda: ctx.forward_image_dev(bad, f1.image, sw, sh, 1), S.ERR_INVALID)
            _err(lambda: ctx.process_image_dev(bad, sw, sh, d1.image, dw, dh, 1), S.ERR_INVALID)
            model_calls_still_good()
        for make in (lambda im: variant(im, ptr=0), lambda im: variant(im, elem=-1), lambda im: variant(im, scale=float("inf")),
                     lambda im: variant(im, stride=im.stride - 3), lambda im: variant(im, px_step=0),      # (a row's reach is stride - 3 here)
                     lambda im: variant(im, ptr=s1.image.ptr), lambda im: variant(im, ptr=s1.image.ptr + 3 * sw * (sh - 1))):      # on the source
            _err(lambda: ctx.forward_image_dev(s1.image, make(f1.image), sw, sh, 1), S.ERR_INVALID)
            _err(lambda: ctx.process_image_dev(s1.image, sw, sh, make(d1.image), dw, dh, 1), S.ERR_INVALID)
            model_calls_still_good()
        _err(lambda: ctx.forward_image_dev(s1.image, f1.image, sw, sh, 0), S.ERR_INVALID)
        _err(lambda: ctx.forward_image_dev(s1.image, f1.image, 0, sh, 1), S.ERR_INVALID)
        _err(lambda: ctx.process_image_dev(s1.image, sw, sh, d1.image, dw, 0, 1), S.ERR_INVALID)
        model_calls_still_good()
        for sizes in ((0, sh, dw, dh), (sw, sh, dw, 0), (-1, sh, dw, dh)):
            _err(lambda: ctx.resize_cubic_image_dev(s.image, sizes[0], sizes[1], d.image, sizes[2], sizes[3], 3, 1), S.ERR_INVALID)
        _err(lambda: ctx.resize_cubic_image_dev(s.image, sw, sh, d.image, dw, dh, 3, 0), S.ERR_INVALID)
        _err(lambda: ctx.resize_cubic_image_dev(s.image, sw, sh, d.image, dw, dh, 0, 1), S.ERR_INVALID)
        # INVALID: process_rgb's own -- shrinking, luma, clamp (past the binding's own checks, through the library)
        lib, h = S.load_library(), ctx._h
        import ctypes as C
        f4, f2_ = lambda *v: (C.c_float * 4)(*v), lambda *v: (C.c_float * 2)(*v)
        rgb = lambda a, asz, b, bsz, luma, clamp: lib.srcnn_process_rgb_image_dev(h, C.byref(a.c()), *asz, C.byref(b.c()), *bsz, luma, clamp, 1)
        assert rgb(d.image, (dw, dh), Buf(fmt, 1, 3, sh, sw, 255.0).image, (sw, sh), f4(*S.LUMA_BT601), None) == S.ERR_INVALID      # shrinks
        assert rgb(s.image, (sw, sh), d.image, (dw, dh), f4(0.5, -0.5, 0.0, 0.0), None) == S.ERR_INVALID
        assert rgb(s.image, (sw, sh), d.image, (dw, dh), f4(float("nan"), 1, 1, 0), None) == S.ERR_INVALID
        assert rgb(s.image, (sw, sh), d.image, (dw, dh), None, None) == S.ERR_INVALID
        assert rgb(s.image, (sw, sh), d.image, (dw, dh), f4(*S.LUMA_BT601), f2_(1.0, 0.0)) == S.ERR_INVALID
        assert rgb(s.image, (sw, sh), d.image, (dw, dh), f4(*S.LUMA_BT601), f2_(float("nan"), 1.0)) == S.ERR_INVALID
        d.parent.fill_(GUARD[R.U8])
        run(ctx.process_rgb_image_dev, s.image, sw, sh, d.image, dw, dh)
        assert np.array_equal(d.get(), want_rgb) and d.guards_intact(), "after the refusals the good call still gives its result"
        # STATE: a colour model in process_rgb; process_image runs it
        ctx.set_model(*random_color_model(1, 3))
        assert "1-channel" in _err(lambda: ctx.process_rgb_image_dev(s.image, sw, sh, d.image, dw, dh), S.ERR_STATE)
        run(ctx.process_image_dev, s.image, sw, sh, d.image, dw, dh, 1)
        _err(lambda: ctx.process_image_dev(variant(s.image, ch_pitch=0), sw, sh, d.image, dw, dh, 1), S.ERR_INVALID)
        still_good()
