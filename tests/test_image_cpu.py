"""Images as they are stored, the parts that need no GPU: the reference conversions against torch's CPU ops, srcnn_image_check,
the header and the exports, the torch front end's tensor-to-descriptor mapping and its refusals, and the listing of the new
kernels of srcnn_pipeline.hip."""
import ctypes as C
import functools
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd import torch_api
import image_reference as R

ROOT = Path(__file__).resolve().parent.parent

# ties, the byte range's ends, negatives, float16's largest value, the last value that rounds to it, the first that overflows,
# subnormals of float16 and float32, infinities, NaN
SPECIAL = np.array([0.0, -0.0, 0.5, 1.5, 2.5, 254.5, 255.0, 255.49, 255.5, 256.0, 1e9, -0.5, -1.0, -1e9, 65504.0, 65519.9, 65520.0,
                    -65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 6e-8, 1e-40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                    1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 3.3895314e38, np.inf, -np.inf, np.nan], dtype=np.float32)


def values():
    rng = np.random.default_rng(5)
    wide = (rng.standard_normal(4096) * 10.0 ** rng.integers(-8, 6, 4096)).astype(np.float32)
    return np.concatenate([SPECIAL, wide, rng.random(4096, dtype=np.float32) * 300 - 20])


# ---- 1: the reference conversions are torch's --------------------------------------------------------------------------------
def test_reference_stores_equal_torch_cpu():
    v = values()
    t = torch.from_numpy(v)
    f16 = t.to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    bf16 = t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert R.same_stored(R.store(v, R.F16), f16, R.F16)
    assert R.same_stored(R.store(v, R.BF16), bf16, R.BF16)
    assert np.array_equal(R.is_nan_bits(R.store(v, R.F16), R.F16), np.isnan(v))
    assert np.array_equal(R.is_nan_bits(R.store(v, R.BF16), R.BF16), np.isnan(v))
    # (a NaN to uint8 is undefined in torch: the library's 0 is asserted below, torch is asked about the rest)
    ok = ~np.isnan(v)
    for scale in (1.0, 255.0, 0.37):
        want = torch.from_numpy(v[ok]).mul(scale).clamp(0, 255).round().to(torch.uint8).numpy()
        assert np.array_equal(R.store(v[ok], R.U8, scale), want), scale
    assert R.store(np.float32([np.nan]), R.U8, 1.0)[0] == 0


def test_reference_store_of_the_named_values():
    u8 = lambda x: int(R.store(np.float32([x]), R.U8, 1.0)[0])
    assert [u8(x) for x in (0.5, 1.5, 2.5, 254.5, 255.5, -3.0, 1e9, np.inf, -np.inf)] == [0, 2, 2, 254, 255, 0, 255, 255, 0]
    f16 = lambda x: R.store(np.float32([x]), R.F16).view(np.float16)[0]
    assert f16(65504.0) == 65504 and f16(65519.9) == 65504 and np.isposinf(f16(65520.0)) and np.isneginf(f16(-65520.0))
    assert f16(2.0 ** -24) == 2.0 ** -24 and f16(2.0 ** -25) == 0 and f16(1.5 * 2.0 ** -24) == 2.0 ** -23      # subnormals, ties
    assert R.store(np.float32([1.0 + 2.0 ** -8]), R.BF16)[0] == 0x3F80 and R.store(np.float32([1.0 + 3 * 2.0 ** -8]), R.BF16)[0] == 0x3F82


def test_reference_loads_equal_torch_cpu():
    rng = np.random.default_rng(6)
    b16 = rng.integers(0, 1 << 16, 5000).astype(np.uint16)
    for elem, dt in ((R.F16, torch.float16), (R.BF16, torch.bfloat16)):
        want = torch.from_numpy(b16.view(np.int16)).view(dt).float().numpy()
        assert R.same_stored(R.load(b16, elem).view(np.uint32), want.view(np.uint32), R.F32)      # (NaN payloads apart)
    b8 = np.arange(256, dtype=np.uint8)
    for scale in (1.0 / 255.0, 1.0, 0.1):
        assert np.array_equal(R.load(b8, R.U8, scale), (torch.from_numpy(b8).float() * scale).numpy())


# ---- 2: srcnn_image_check, no context -------------------------------------------------------------------------------------
def img(ptr=0x10000, elem=S.ELEM_F32, px=1, stride=0, ch=0, frame=0, scale=1.0):
    return S.Image(ptr, elem, px, stride, ch, frame, scale)


def test_image_check_accepts_the_layouts():
    w, h = 10, 5
    for dst in (False, True):
        assert S.image_check(img(stride=w, ch=w * h, frame=3 * w * h), w, h, 3, 2, dst)                                  # NCHW
        assert S.image_check(img(elem=S.ELEM_F16, px=3, stride=3 * w, ch=1, frame=3 * w * h), w, h, 3, 2, dst)            # NHWC
        assert S.image_check(img(elem=S.ELEM_U8, px=4, stride=4 * w, ch=1, frame=4 * w * h, scale=255.0), w, h, 3, 2, dst)  # RGBA
        assert S.image_check(img(elem=S.ELEM_U8, px=3, stride=3 * w), w, h, 1, 1, dst)                   # one interleaved channel
        assert S.image_check(img(elem=S.ELEM_BF16, stride=w + 7, ch=(w + 7) * h + 3, frame=3 * ((w + 7) * h + 3) + 11), w, h, 3, 2, dst)
        assert S.image_check(img(ptr=0x10001, elem=S.ELEM_U8), 1, 1, 1, 1, dst)         # every pitch ignored, an odd address
        assert S.image_check(img(stride=w, ch=0, frame=0), w, h, 1, 1, dst)             # pitches whose count is 1: ignored


def test_image_check_refusals():
    w, h = 10, 5
    good = dict(stride=w, ch=w * h, frame=3 * w * h)
    lib = S.load_library()
    assert lib.srcnn_image_check(None, w, h, 3, 1, 0) == S.ERR_INVALID
    assert not S.image_check(img(ptr=0, **good), w, h, 3)
    for elem in (-1, 4, 99):
        assert not S.image_check(img(elem=elem, **good), w, h, 3)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert not S.image_check(img(elem=S.ELEM_U8, scale=scale, **good), w, h, 3)
        assert S.image_check(img(elem=S.ELEM_F16, scale=scale, **good), w, h, 3), "the scale is ignored but for U8"
    for size in ((0, h, 3, 1), (w, 0, 3, 1), (w, h, 0, 1), (w, h, 3, 0), (-1, h, 3, 1)):
        assert not S.image_check(img(**good), *size)
    for zero in ("px", "stride", "ch", "frame"):           # a used step of 0, source or destination
        kw = dict(px=1, **good)
        kw[zero] = 0
        assert not S.image_check(img(**kw), w, h, 3, 2)
    assert not S.image_check(img(stride=1 << 62, ch=1, px=2), 2, 8, 2)                      # last offset beyond 63 bits
    assert not S.image_check(img(stride=(1 << 61) // 4, ch=1, px=2), 2, 8 * 4 + 1, 2)      # ... in BYTES
    assert S.image_check(img(elem=S.ELEM_U8, stride=1 << 50, ch=1, px=2), 2, 8, 2)
    assert not S.image_check(img(ptr=0x10002, **good), w, h, 3) and not S.image_check(img(ptr=0x10001, elem=S.ELEM_F16, **good), w, h, 3)
    assert S.image_check(img(ptr=0x10002, elem=S.ELEM_BF16, **good), w, h, 3) and S.image_check(img(ptr=0x10004, **good), w, h, 3)


def test_injectivity_rule_at_and_below_its_bound():
    w, h = 10, 5
    # interleaved 3-channel rows: the last element of a row is at 2 + 9 * 3 = 29, so the stride must exceed 29
    at, below = img(px=3, stride=30, ch=1), img(px=3, stride=29, ch=1)
    assert S.image_check(at, w, h, 3, 1, True) and not S.image_check(below, w, h, 3, 1, True)
    assert S.image_check(below, w, h, 3, 1, False), "a source may alias itself"
    # planar: channel pitch against the plane's reach, frame pitch against the frame's
    reach = (h - 1) * w + (w - 1)
    assert S.image_check(img(stride=w, ch=reach + 1, frame=10000), w, h, 3, 2, True)
    assert not S.image_check(img(stride=w, ch=reach, frame=10000), w, h, 3, 2, True)
    frame_reach = 2 * (reach + 1) + reach
    assert S.image_check(img(stride=w, ch=reach + 1, frame=frame_reach + 1), w, h, 3, 2, True)
    assert not S.image_check(img(stride=w, ch=reach + 1, frame=frame_reach), w, h, 3, 2, True)
    # frames inside the channel pitch (channels of frames) are as good as channels inside the frame pitch
    assert S.image_check(img(stride=w, frame=reach + 1, ch=2 * (reach + 1)), w, h, 3, 2, True)
    assert not S.image_check(img(px=1, stride=w - 1), w, h, 1, 1, True) and S.image_check(img(px=1, stride=w - 1), w, h, 1, 1, False)
    assert not S.image_check(img(px=3, stride=30, ch=3), w, h, 2, 1, True), "a channel pitch equal to the pixel step"


# ---- 3: header, exports, ABI version -----------------------------------------------------------------------------------------
NEW_SYMBOLS = ("srcnn_image_check", "srcnn_forward_image_dev", "srcnn_resize_cubic_image_dev", "srcnn_process_image_dev",
               "srcnn_process_rgb_image_dev")


def test_header_declares_documents_and_scopes_the_new_calls():
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    blocks = re.findall(r"/\*.*?\*/", text, flags=re.S)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    mine = [b for b in blocks if "srcnn_image_check" in b]
    assert mine
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", code), name
        assert any(name in b for b in mine), name
        assert name in S.ABI_SYMBOLS
    assert re.search(r"typedef struct srcnn_image \{[^}]*void\s*\*data;[^}]*int\s+elem;[^}]*float\s+scale;[^}]*size_t px_step, stride, "
                     r"ch_pitch, frame_pitch;", code)
    assert re.search(r"SRCNN_ELEM_F32 = 0, SRCNN_ELEM_F16 = 1, SRCNN_ELEM_BF16 = 2, SRCNN_ELEM_U8 = 3", code)
    for said in ("bit for bit", "Out of scope", "host-memory forms", "row stripes and several GPUs", "byte entry points", "uint16",
                 "command-line option", "injective", "srcnn_set_input_range", "nearest even"):
        assert any(said in b for b in mine), said
    assert (S.ELEM_F32, S.ELEM_F16, S.ELEM_BF16, S.ELEM_U8) == (0, 1, 2, 3)


def test_the_library_exports_the_new_calls_and_the_abi_version_stays():
    lib = S.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.srcnn_abi_version() == 1
    assert C.sizeof(S._CImage) == 48


# ---- 4: the torch mapping, on CPU tensors -------------------------------------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def fields(im):
    return im.elem, im.px_step, im.stride, im.ch_pitch, im.frame_pitch


def test_descriptor_of_stored_tensors():
    hwc = np.zeros((5, 7, 3), np.uint8)
    t = torch.from_numpy(hwc).permute(2, 0, 1)
    im, n, h, w = torch_api.describe_image(t, 3)
    assert (n, h, w) == (1, 5, 7) and fields(im) == (S.ELEM_U8, 3, 21, 1, 0) and im.ptr == t.data_ptr()
    assert im.scale == 1.0 / 255.0 and torch_api.is_channels_last(im, 3)
    assert torch_api.describe_image(t, 3, in_scale=0.5)[0].scale == 0.5
    x = torch.zeros(2, 3, 5, 7, dtype=torch.float16).to(memory_format=torch.channels_last)
    im, n, h, w = torch_api.describe_image(x, 3)
    assert (n, h, w) == (2, 5, 7) and fields(im) == (S.ELEM_F16, 3, 21, 1, 105) and torch_api.is_channels_last(im, 3)
    parent = torch.zeros(2, 4, 9, 16, dtype=torch.bfloat16)
    rows = parent[:, :3, 2:7, 3:10]                                       # row-strided
    im, n, h, w = torch_api.describe_image(rows, 3)
    assert fields(im) == (S.ELEM_BF16, 1, 16, 144, 576) and im.ptr == parent.data_ptr() + 2 * (2 * 16 + 3)
    assert not torch_api.is_channels_last(im, 3)
    chans = torch.zeros(6, 5, 7)[::2]                                      # channel-strided, float32
    assert fields(torch_api.describe_image(chans, 3)[0]) == (S.ELEM_F32, 1, 7, 70, 0)
    one = torch.zeros(5, 7, 3, dtype=torch.uint8).permute(2, 0, 1)[1:2]   # one channel of an interleaved image
    assert fields(torch_api.describe_image(one, 1)[0]) == (S.ELEM_U8, 3, 21, 0, 0)
    for im_, shape in ((torch_api.describe_image(t, 3)[0], (3, 5, 7)), (torch_api.describe_image(x, 3)[0], (3, 5, 7))):
        assert S.image_check(im_, 7, 5, 3, 1, True)


def test_empty_image_allocates_what_was_asked():
    x = torch.zeros(2, 3, 5, 7)
    out, im = torch_api.empty_image(x, 2, 3, 10, 14, torch.uint8, True)
    assert out.shape == (2, 3, 10, 14) and out.dtype == torch.uint8 and out.stride() == (420, 1, 42, 3)
    assert fields(im) == (S.ELEM_U8, 3, 42, 1, 420) and im.scale == 255.0
    out, im = torch_api.empty_image(x[0], 1, 3, 10, 14, torch.float16, False)
    assert out.shape == (3, 10, 14) and out.is_contiguous() and fields(im) == (S.ELEM_F16, 1, 14, 140, 420)
    with pytest.raises(ValueError):
        torch_api.empty_image(x, 2, 3, 10, 14, torch.float64, False)
    with pytest.raises(ValueError):
        torch_api.empty_image(x, 2, 3, 10, 14, torch.uint8, False, out_scale=0.0)


def test_torch_methods_refuse_before_the_library():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 3, 0, None
    good = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    calls = (lambda t, **k: fast.forward_image(t, **k), lambda t, **k: fast.resize_image(t, (16, 16), **k),
             lambda t, **k: fast.upscale_image(t, scale=2, **k))
    for call in calls:
        with pytest.raises(ValueError, match="float32, float16, bfloat16 or uint8"):
            call(good.double())
        with pytest.raises(ValueError, match="channel"):
            call(torch.zeros(1, 4, 8, 8))                                 # wrong channel count
        with pytest.raises(ValueError, match="channel"):
            call(torch.zeros(8, 8, 3))                                    # H x W x C is not guessed
        with pytest.raises(ValueError, match="shape"):
            call(torch.zeros(8, 8))
        with pytest.raises(ValueError, match="empty"):
            call(torch.zeros(1, 3, 0, 8))
        with pytest.raises(ValueError, match="stride"):
            call(torch.zeros(1, 3, 8, 8).expand(2, 3, 8, 8))              # frames on top of each other
        with pytest.raises(ValueError, match="in_scale"):
            call(good, in_scale=0.0)
        with pytest.raises(ValueError, match="cuda"):
            call(good)                                                    # a CPU tensor: there is no CPU path
        with pytest.raises(ValueError, match="not a tensor|torch.Tensor"):
            call(np.zeros((3, 8, 8), np.float32))
    with pytest.raises(ValueError, match="exactly one"):
        fast.upscale_image(good)
    with pytest.raises(ValueError, match="exactly one"):
        fast.upscale_image(good, scale=2, size=(16, 16))
    with pytest.raises(ValueError, match="1-channel"):
        fast.upscale_rgb_image(good, scale=2)                             # a colour module
    luma = object.__new__(torch_api.CompiledModule)
    luma.ctx, luma.channels, luma.device, luma._side = _NoCall(), 1, 0, None
    with pytest.raises(ValueError, match="smaller"):
        luma.upscale_rgb_image(good, size=(4, 16))
    with pytest.raises(ValueError):
        luma.upscale_rgb_image(good, scale=2, luma=(0.0, 0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        luma.upscale_rgb_image(good, scale=2, clamp=(1.0, 0.0))
    with pytest.raises(ValueError, match="cuda"):
        luma.upscale_rgb_image(good, scale=2)
    with pytest.raises(ValueError, match="channel"):
        luma.upscale_rgb_image(torch.zeros(1, 1, 8, 8), scale=2)
    if torch.cuda.is_available() and torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="cuda:0"):
            fast.forward_image(good.to("cuda:1"))


def test_existing_methods_still_refuse_stored_formats():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 3, 0, None
    with pytest.raises(ValueError, match="expected a float32 tensor"):
        fast(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"call \.contiguous\(\)"):
        fast(torch.zeros(1, 3, 8, 8).to(memory_format=torch.channels_last))


# ---- 5: the listing -------------------------------------------------------------------------------------------------------
UNIT = "srcnn_pipeline.hip"
TILE_LDS = 4 * 20 * (256 + 264)
NEW_KERNELS = {"resize_cubic_image_direct_kernel": 0, "resize_cubic_image_tiled_kernel": TILE_LDS, "luma_resize_image_kernel": TILE_LDS,
               "resize_merge_image_kernel": TILE_LDS, "resize_merge_image_pixels_kernel": TILE_LDS, "convert_image_kernelILi1E": 0,
               "convert_image_kernelILi3E": 0}


@functools.lru_cache(maxsize=None)
def pipeline_listing():
    flags = [u[1] for u in B.UNITS if u[0] == UNIT and len(u) == 2][0]
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "unit.s"
        subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, f"-I{B.CSRC}", "-S", "--cuda-device-only",
                        "-o", str(out), str(B.CSRC / UNIT)], check=True, stderr=subprocess.DEVNULL)
        text = out.read_text()
    return dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)), text


@pytest.mark.parametrize("kernel", sorted(NEW_KERNELS))
def test_new_pipeline_kernels_use_no_scratch_and_keep_the_tile(kernel):
    descs, text = pipeline_listing()
    mine = [n for n in descs if kernel in n]
    assert len(mine) == 1, mine
    field = lambda f: int(re.search(rf"\.amdhsa_{f} (\d+)", descs[mine[0]]).group(1))
    assert field("private_segment_fixed_size") == 0
    meta = re.search(rf"\.name:\s+{re.escape(mine[0])}\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert meta and int(meta.group(1)) == 0
    assert field("group_segment_fixed_size") == NEW_KERNELS[kernel]
    body = re.search(rf"^{re.escape(mine[0])}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M).group(1)
    assert not re.search(r"\bv_(fma|fmac|mad|mac)_f32\b", body), "no contraction: every product and sum is rounded on its own"
    # the old names stay unique: the existing listing tests look for exactly one kernel per substring
    for old in ("luma_resize_f32_kernel", "resize_merge_f32_kernel", "resize_cubic_f32_tiled_kernel"):
        assert old not in mine[0] and sum(old in n for n in descs) == 1
