"""CPU tests of srcnn_process_rgb_f32* (a 3-plane float image through a 1-channel model): no device.
1. the formula the call computes, out_c = up(x_c) + g (Ysr - Yup), against the program it replaces -- a float64 round trip
   through the full Y'CbCr matrix and its exact inverse -- for three colour conventions and a nonlinear stand-in model;
2. srcnn_luma_gain -- host only -- against the float64 value rounded once, and its refusals;
3. the Python binding and the torch front end refuse bad arguments before any call into the library;
4. include/srcnn_amd.h documents and declares every new symbol;
5. the two new kernels of srcnn_pipeline.hip, compiled with the build's flags, keep nothing in scratch memory and use the
   resize's tile."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd import torch_api
from rgb_f32_reference import CONVENTIONS, BT601_FULL, classic64, formula64, gain64, luma_lr_f32, merge_f32, rgb, standin_model

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def built():
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return S.load_library()


# ---- 1: the arithmetic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conv", CONVENTIONS, ids=lambda c: c.name)
@pytest.mark.parametrize("sh,sw,dh,dw", [(5, 4, 10, 8), (17, 33, 25, 49), (12, 9, 12, 9)])
def test_formula_equals_the_classic_round_trip(conv, sh, sw, dh, dw):
    assert np.abs(conv.matrix[1:].sum(axis=1)).max() < 1e-12, "the chroma rows sum to zero: what the formula rests on"
    x = rgb((3, sh, sw), 7 * sh + dw)
    want = classic64(x, dh, dw, conv, standin_model)
    got = formula64(x, dh, dw, conv.luma(), standin_model)
    diff = np.abs(got - want).max()
    print(f"{conv.name} {sh}x{sw} -> {dh}x{dw}: max|formula - classic| = {diff:.3g}")
    assert diff <= 1e-12
    assert np.abs(want - np.asarray(x, np.float64).mean()).max() > 0.05, "the stand-in model changes the image"


def test_float32_statement_follows_the_float64_formula():
    """luma_lr_f32 / merge_f32 -- what the GPU tests compose with existing calls -- are the formula's steps 1 and 4."""
    x = rgb((3, 9, 11), 3)
    luma = BT601_FULL.luma()
    y = luma_lr_f32(x, luma)
    w = np.float64(np.float32(luma))
    assert np.abs(y - (w[0] * x[0] + w[1] * x[1] + w[2] * x[2] + w[3])).max() <= 4 * 2.0 ** -24
    u, ysr, yup = rgb((3, 6, 5), 4), rgb((6, 5), 5) * np.float32(1.5), rgb((6, 5), 6)
    g = np.float32(gain64(luma))
    free = merge_f32(u, ysr, yup, g)
    assert np.abs(free - (np.float64(u) + (np.float64(ysr) - yup) * g)).max() <= 4 * 2.0 ** -24 * 3
    assert free.min() < 0.0 and free.max() > 1.0
    bound = merge_f32(u, ysr, yup, g, (0.0, 1.0))
    assert bound.min() == 0.0 and bound.max() == 1.0
    inside = (free >= 0) & (free <= 1)
    assert np.array_equal(bound[inside], free[inside])
    u[0, 0, 0] = np.nan
    assert np.isnan(merge_f32(u, ysr, yup, g, (0.0, 1.0))[0, 0, 0]), "a NaN is not clamped away"


# ---- 2: srcnn_luma_gain -----------------------------------------------------------------------------------------------------
def _gain(lib, luma):
    a, g = (C.c_float * 4)(*luma), C.c_float(-1.0)
    return lib.srcnn_luma_gain(a, C.byref(g)), g.value


@pytest.mark.parametrize("luma", [c.luma() for c in CONVENTIONS] + [S.LUMA_BT601, S.luma_bt601_studio(255.0), (1.0, 2.0, 4.0, -3.0),
                                                                   (0.1, 0.1, 0.1, 0.0), (3e-5, 1e-5, -2e-5, 1.0)])
def test_luma_gain_is_the_float64_value_rounded_once(built, luma):
    rc, g = _gain(built, luma)
    assert rc == 0
    assert np.float32(g) == np.float32(gain64(luma))
    assert S.luma_gain(luma) == g


def test_luma_gain_refusals(built):
    g = C.c_float()
    good = (C.c_float * 4)(0.299, 0.587, 0.114, 0.0)
    assert built.srcnn_luma_gain(None, C.byref(g)) == S.ERR_INVALID
    assert built.srcnn_luma_gain(good, None) == S.ERR_INVALID
    for bad in ((float("nan"), 0.5, 0.5, 0.0), (0.3, float("inf"), 0.1, 0.0), (0.3, 0.6, 0.1, float("nan")),
                (0.3, 0.6, 0.1, float("-inf")), (0.0, 0.0, 0.0, 0.0), (0.5, -0.25, -0.25, 0.0), (-0.3, -0.6, -0.1, 0.0)):
        rc, value = _gain(built, bad)
        assert rc == S.ERR_INVALID and value == -1.0, bad
        with pytest.raises(ValueError):
            S.luma_gain(bad)
    for bad in ((0.3, 0.6, 0.1), (0.3, 0.6, 0.1, 0.0, 0.0), None, "bt601", 0.3):
        with pytest.raises(ValueError):
            S.luma_gain(bad)
    assert built.srcnn_abi_version() == 1


def test_presets():
    assert S.LUMA_BT601 == (0.299, 0.587, 0.114, 0.0)
    assert S.luma_bt601_studio(1.0) == (65.481 / 255, 128.553 / 255, 24.966 / 255, 16 / 255)
    assert S.luma_bt601_studio(255.0)[3] == 16.0 and S.luma_bt601_studio(255.0)[:3] == S.luma_bt601_studio(1.0)[:3]
    assert S.luma_for_order(S.LUMA_BT601, "bgr") == (0.114, 0.587, 0.299, 0.0)
    assert S.luma_for_order((1.0, 2.0, 3.0, 4.0), "bgr") == (3.0, 2.0, 1.0, 4.0)
    assert S.luma_for_order(S.LUMA_BT601, "rgb") == S.LUMA_BT601
    with pytest.raises(ValueError):
        S.luma_for_order(S.LUMA_BT601, "grb")


# ---- 3: refusals in Python, before any call into the library --------------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


BAD_LUMAS = [(0.3, 0.6, 0.1), (float("nan"), 0.6, 0.1, 0.0), (0.3, 0.6, 0.1, float("inf")), (0.0, 0.0, 0.0, 0.0), (-1.0, 0.5, 0.25, 0.0),
             None, "bt601"]
BAD_CLAMPS = [(1.0, 0.0), (float("nan"), 1.0), (0.0, float("nan")), (0.0,), (0.0, 1.0, 2.0), 1.0]


def test_python_binding_refuses_before_the_library():
    ctx = object.__new__(S.Context)           # no device needed: only the Python-side validation runs
    ctx._lib, ctx._h = _NoCall(), None
    good = np.zeros((3, 8, 8), np.float32)
    call = ctx.process_rgb_f32
    with pytest.raises(TypeError):
        call(good.astype(np.float64), 16, 16)                    # wrong dtype
    with pytest.raises(TypeError):
        call(np.zeros((3, 8, 8), np.uint8), 16, 16)
    with pytest.raises(TypeError):
        call(np.zeros((1, 3, 8, 8), np.float32), 16, 16)         # wrong rank
    with pytest.raises(TypeError):
        call([[0.0]], 16, 16)                                    # not an array
    for wrong in (np.zeros((8, 8), np.float32), np.zeros((1, 8, 8), np.float32), np.zeros((4, 8, 8), np.float32)):
        with pytest.raises(ValueError):
            call(wrong, 16, 16)                                  # not three planes
    with pytest.raises(ValueError):
        call(np.zeros((3, 8, 16), np.float32)[:, :, ::2], 16, 16)        # rows not contiguous
    with pytest.raises(ValueError):
        call(np.zeros((3, 0, 8), np.float32), 16, 16)            # empty
    for bad in ((0, 16), (16, -1), (16.0, 16), (True, 16), (7, 16), (16, 7)):      # the last two shrink one axis
        with pytest.raises(ValueError):
            call(good, *bad)
    for bad in BAD_LUMAS:
        with pytest.raises(ValueError):
            call(good, 16, 16, luma=bad)
        with pytest.raises(ValueError):
            ctx.process_rgb_f32_dev(64, 8, 64, 0, 8, 8, 4096, 16, 256, 0, 16, 16, luma=bad)
    for bad in BAD_CLAMPS:
        with pytest.raises(ValueError):
            call(good, 16, 16, clamp=bad)
        with pytest.raises(ValueError):
            ctx.process_rgb_f32_dev(64, 8, 64, 0, 8, 8, 4096, 16, 256, 0, 16, 16, clamp=bad)
    with pytest.raises(ValueError):
        ctx.process_rgb_f32_dev(64, 8, 64, 0, 8, 8, 4096, 16, 256, 0, 16, 7)          # shrinks


def test_torch_front_end_refuses_before_the_library():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 1, 0, None
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="exactly one"):
        fast.upscale_rgb(x)                                              # neither
    with pytest.raises(ValueError, match="exactly one"):
        fast.upscale_rgb(x, scale=2, size=(16, 16))                      # both
    for call in (lambda t: fast.upscale_rgb(t, size=(16, 16)), lambda t: fast.upscale_rgb(t, scale=2)):
        with pytest.raises(ValueError):
            call(x.double())                                             # wrong dtype
        with pytest.raises(ValueError):
            call(torch.zeros(8, 8))                                      # wrong rank
        with pytest.raises(ValueError):
            call(torch.zeros(1, 1, 8, 8))                                # one plane: that is upscale()
        with pytest.raises(ValueError):
            call(x)                                                      # a CPU tensor: there is no CPU path
    colour = object.__new__(torch_api.CompiledModule)
    colour.ctx, colour.channels, colour.device, colour._side = _NoCall(), 3, 0, None
    with pytest.raises(ValueError, match="1-channel"):
        colour.upscale_rgb(x, scale=2)                                   # a colour module: upscale() runs that one
    if torch.cuda.is_available():          # past check_input only a CUDA tensor goes: the remaining refusals need one
        xc = torch.zeros(1, 3, 8, 8, device="cuda")
        for bad in ((16,), (0, 16), (16, 2.5), 16, (7, 16), (16, 7)):
            with pytest.raises(ValueError):
                fast.upscale_rgb(xc, size=bad)
        for bad in BAD_LUMAS:
            with pytest.raises(ValueError):
                fast.upscale_rgb(xc, scale=2, luma=bad)
        for bad in BAD_CLAMPS:
            with pytest.raises(ValueError):
                fast.upscale_rgb(xc, scale=2, clamp=bad)


# ---- 4: the header ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("srcnn_luma_gain", "srcnn_process_rgb_f32", "srcnn_process_rgb_f32_dev")


def test_header_documents_and_declares_every_new_symbol():
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    blocks = re.findall(r"/\*.*?\*/", text, flags=re.S)
    comments = " ".join(blocks)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", code), f"{name} is declared"
        assert re.search(rf"\b{name}\b", comments), f"{name} is documented"
        assert name in S.ABI_SYMBOLS
    for said in ("SRCNN_MODE_BANDED16", "srcnn_set_input_range", "bit for bit", "w0 + w1 + w2", "shrink"):
        assert any(said in b for b in blocks if "srcnn_luma_gain" in b), said


# ---- 5: the listing ---------------------------------------------------------------------------------------------------------
UNIT = "srcnn_pipeline.hip"


@functools.lru_cache(maxsize=None)
def pipeline_kernels():
    """{mangled name: kernel descriptor} of the unit, compiled with the build's flags for it."""
    import tempfile
    flags = [u[1] for u in B.UNITS if u[0] == UNIT and len(u) == 2][0]
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "unit.s"
        subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, f"-I{B.CSRC}", "-S", "--cuda-device-only",
                        "-o", str(out), str(B.CSRC / UNIT)], check=True, stderr=subprocess.DEVNULL)
        text = out.read_text()
    return dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)), text


@pytest.mark.parametrize("kernel", ["luma_resize_f32_kernel", "resize_merge_f32_kernel"])
def test_new_kernels_use_no_scratch_and_the_resizes_tile(kernel):
    descs, text = pipeline_kernels()
    mine = [n for n in descs if kernel in n]
    assert len(mine) == 1, mine
    tiled = [n for n in descs if "resize_cubic_f32_tiled_kernel" in n]
    assert len(tiled) == 1
    field = lambda n, f: int(re.search(rf"\.amdhsa_{f} (\d+)", descs[n]).group(1))
    assert field(mine[0], "private_segment_fixed_size") == 0
    meta = re.search(rf"\.name:\s+{re.escape(mine[0])}\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert meta and int(meta.group(1)) == 0
    # the tile of the resize, unchanged: 20 x 256 + 20 x 264 floats, three workgroups per CU
    assert field(mine[0], "group_segment_fixed_size") == field(tiled[0], "group_segment_fixed_size") == 4 * 20 * (256 + 264)
