"""Pillow's resize of uint8 images (srcnn_resize_pil_image_dev), the part that needs no GPU:
1. the numpy restatement (tests/pil_reference.py) against Pillow itself, byte for byte, and against Pillow's committed results;
2. srcnn_pil_taps against the restatement, exact in first, count and every coefficient; the sizing call and every refusal;
3. teeth: the two wrong implementations the bitwise GPU tests must catch do differ from Pillow;
4. the shape list holds the kernels' tile bounds as srcnn_image.h declares them;
5. header text, exports, ABI version; the Python and torch layers refuse before the library;
6. srcnn_pil_taps under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program (tests/checks/san_pil_taps.cpp).
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
from srcnn_cpp_amd import torch_api
import pil_reference as R

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "pil_resize_golden.npz"
AXES = sorted({(sw, dw) for _, sw, _, dw in R.all_shapes()} | {(sh, dh) for sh, _, dh, _ in R.all_shapes()} |
              {(1920, 3840), (3840, 1920), (1080, 2160)})
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def built():
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return S.load_library()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- 1: the restatement against Pillow -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.all_shapes(), ids=ids)
def test_restatement_equals_pillow_byte_for_byte(shape):
    Image = pytest.importorskip("PIL.Image")
    sh, sw, dh, dw = shape
    for name, img in R.inputs(sh, sw).items():
        for fname, f in R.FILTERS.items():
            want = np.asarray(Image.fromarray(img).resize((dw, dh), Image.Resampling(f)))
            got = R.resize(img, dh, dw, f)
            assert got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), f"{name} {fname}: {(got != want).mean():.3%} of the bytes differ"


@pytest.mark.parametrize("shape", R.all_shapes(), ids=ids)
def test_restatement_equals_the_committed_pillow_results(golden, shape):
    sh, sw, dh, dw = shape
    for name, img in R.inputs(sh, sw).items():
        assert np.array_equal(img, golden[f"in/{sh}x{sw}/{name}"]), "the committed results were made from these inputs"
        for fname, f in R.FILTERS.items():
            assert np.array_equal(R.resize(img, dh, dw, f), golden[f"out/{sh}x{sw}-{dh}x{dw}/{name}/{fname}"]), (name, fname)


def test_the_checkerboard_saturates_at_both_ends(golden):
    hit = {0: 0, 255: 0}
    for sh, sw, dh, dw in [(23, 37, 46, 74), (61, 97, 30, 48)]:
        img = R.inputs(sh, sw)["checker"]
        t = R.taps(sw, dw, R.BICUBIC)
        acc = R._pass_sums(img[None], *t) >> R.PRECISION_BITS
        hit[0] += int((acc < 0).sum())
        hit[255] += int((acc > 255).sum())
    assert hit[0] > 0 and hit[255] > 0, "the horizontal pass overshoots below 0 and above 255 on the checkerboard"


def test_the_golden_file_is_small_and_complete(golden):
    assert GOLDEN.stat().st_size < (1 << 20)
    sources = {s[:2] for s in R.all_shapes()}      # the inputs are kept once per source size
    assert len(golden) == 1 + 3 * len(sources) + len(R.all_shapes()) * 3 * len(R.FILTERS)


# ---- 2: the library's table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", AXES, ids=ids)
@pytest.mark.parametrize("fname", sorted(R.FILTERS))
def test_table_equals_the_restatement_exactly(built, axis, fname):
    s, n = axis
    first, count, coef = S.pil_taps(s, n, R.FILTERS[fname])
    f0, c0, w0 = R.taps(s, n, R.FILTERS[fname])
    assert first.dtype == np.int32 and count.dtype == np.int32 and coef.dtype == np.int32
    assert np.array_equal(first, f0) and np.array_equal(count, c0)
    assert coef.shape == w0.shape and np.array_equal(coef, w0)
    assert (first >= 0).all() and (first + count <= s).all(), "no index is ever clamped"
    assert np.abs(coef.astype(np.int64)).sum(axis=1).max() < 2 ** 23, "the bound behind the int32 sums (DESIGN.md 4.22)"


def test_filter_numbers_are_pillows():
    Image = pytest.importorskip("PIL.Image")
    assert (S.PIL_BILINEAR, S.PIL_BICUBIC) == (int(Image.Resampling.BILINEAR), int(Image.Resampling.BICUBIC)) == (2, 3)
    assert (R.BILINEAR, R.BICUBIC) == (S.PIL_BILINEAR, S.PIL_BICUBIC)


def test_table_query_form_and_refusals(built):
    ip, cp = C.POINTER(C.c_int), C.POINTER(C.c_int32)
    taps = built.srcnn_pil_taps
    # coef == NULL sizes the table, first and count may be NULL; 62 is the largest count (Pillow allocates ksize = 63 per row)
    assert taps(200, 13, S.PIL_BICUBIC, None, None, None, 0) == 62
    assert taps(37, 74, S.PIL_BICUBIC, None, None, None, 0) == 4 and taps(37, 74, S.PIL_BILINEAR, None, None, None, 0) == 2
    n, k = 13, 62
    first, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    wide = np.full((n, k + 2), -7, np.int32)
    assert taps(200, n, S.PIL_BICUBIC, first.ctypes.data_as(ip), count.ctypes.data_as(ip), wide.ctypes.data_as(cp), k + 2) == k
    f0, c0, w0 = R.taps(200, n, R.BICUBIC)
    assert np.array_equal(wide[:, :k], w0) and (wide[:, k:] == 0).all(), "entries beyond a sample's count are zero-filled"
    assert all((wide[d, count[d]:] == 0).all() for d in range(n))
    fp, kp, wp = first.ctypes.data_as(ip), count.ctypes.data_as(ip), wide.ctypes.data_as(cp)
    for bad in [(0, n, 3, fp, kp, wp, k), (200, 0, 3, fp, kp, wp, k), (-1, n, 3, None, None, None, 0), (200, -5, 2, None, None, None, 0),
                (200, n, 1, fp, kp, wp, k), (200, n, 4, None, None, None, 0), (200, n, 0, fp, kp, wp, k),      # lanczos, hamming, box, nearest
                (200, n, 5, fp, kp, wp, k), (200, n, 3, None, kp, wp, k), (200, n, 3, fp, None, wp, k), (200, n, 3, fp, kp, wp, k - 1)]:
        assert taps(*bad) == S.ERR_INVALID, bad[:3]
    for bad in [(0, 4, 3), (4, 0, 3), (4, 4, 1), (4, 4, "bicubic")]:
        with pytest.raises(ValueError):
            S.pil_taps(*bad)


# ---- 3: teeth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", ["unrounded", "vertical_first"])
@pytest.mark.parametrize("shape", [(23, 37, 46, 74), (61, 97, 20, 32)], ids=ids)
def test_the_two_wrong_implementations_differ_from_pillow(golden, wrong, shape):
    sh, sw, dh, dw = shape
    img = R.inputs(sh, sw)["random"]
    want = golden[f"out/{sh}x{sw}-{dh}x{dw}/random/bicubic"]
    share = (R.resize(img, dh, dw, R.BICUBIC, wrong=wrong) != want).mean()
    print(f"{wrong} on {shape}: {share:.1%} of the bytes differ")
    assert share >= 0.05, "a kernel that does this fails the bitwise tests"


# ---- 4: the shape list and the tile bounds ---------------------------------------------------------------------------------
def test_the_shape_list_holds_the_tile_bounds_of_the_source_text():
    bounds = R.tile_bounds()
    assert bounds == R.EXPECTED_BOUNDS, "a tile bound changed: update EXPECTED_BOUNDS and BOUND_SHAPES in tests/pil_reference.py"
    assert R.bound_shapes(bounds) == R.BOUND_SHAPES
    for name, rows in (("PIL_TR", 2), ("PIL_TC", 3), ("PIL_HC", 3)):
        have = {s[rows] for s in R.BOUND_SHAPES}
        assert {bounds[name] - 1, bounds[name], bounds[name] + 1} <= have, name
    text = (ROOT / "srcnn_cpp_amd" / "csrc" / "srcnn_pipeline.hip").read_text()
    for use in ("hbuf[PIL_RMAX][PIL_TC]", "blockIdx.x * PIL_TC", "rt * PIL_TR", "blockIdx.x * PIL_HC", "__launch_bounds__(PIL_HC)"):
        assert use in text, f"the kernels no longer take their tile from {use}"


def test_listed_issue_shapes_are_all_there():
    assert len(R.SHAPES) == 15 and all(sh * sw < 10000 and dh * dw < 20000 for sh, sw, dh, dw in R.SHAPES)
    assert (9, 200, 9, 13) in R.SHAPES and S.pil_taps(200, 13)[1].max() == 62 > 17      # beyond the tiled form's tap limit


# ---- 5: header, exports, ABI; the layers above refuse before the library ---------------------------------------------------
NEW_SYMBOLS = ["srcnn_pil_taps", "srcnn_resize_pil_image_dev", "srcnn_process_pil_image_dev", "srcnn_process_rgb_pil_image_dev"]


def test_header_exports_and_abi(built):
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    for needle in ("Pillow wins", "center = (d + 0.5) * scale", "xmin = (int)(center - support + 0.5)",
                   "w_j = k((j + xmin - center + 0.5) * (1 / fs))", "if ww != 0: w_j = w_j / ww",
                   "c_j = w_j < 0 ? (int)(-0.5 + w_j * 4194304) : (int)(0.5 + w_j * 4194304)", "acc = 1 << 21",
                   "out = min(max(acc >> 22, 0), 255)", "(((x - 5) * x + 8) * x - 4) * a", "rest on the host's libm",
                   "SRCNN_PIL_BILINEAR = 2, SRCNN_PIL_BICUBIC = 3"):
        assert needle in text, needle
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in exported and name in S.ABI_SYMBOLS and hasattr(built, name), name
    assert not any("resample_pil" in n for n in exported), "the hooks and the launchers stay out of the product"
    assert built.srcnn_abi_version() == 1
    design = (ROOT / "DESIGN.md").read_text()
    assert "4.22" in design and "Where this text and Pillow disagree, Pillow wins" in design


class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


def test_torch_methods_refuse_before_the_library():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 1, 0, None
    u8 = torch.zeros(1, 1, 8, 8, dtype=torch.uint8)
    for method, args in (("resize_pil", ((16, 16),)), ("upscale_pil", ()), ("upscale_rgb_pil", ())):
        kw = {} if method == "resize_pil" else {"scale": 2}
        for dtype in (torch.float32, torch.float16, torch.float64):
            with pytest.raises(TypeError, match=r"resize\(\.\.\., antialias=True\)"):
                getattr(fast, method)(u8.to(dtype), *args, **kw)
        for bad in ("lanczos", 3, None, "BICUBIC"):
            with pytest.raises(ValueError, match="filter"):
                getattr(fast, method)(u8, *args, filter=bad, **kw)
    with pytest.raises(ValueError, match=r"there is no CPU path"):
        fast.resize_pil(u8, (16, 16))
    with pytest.raises(ValueError, match=r"there is no CPU path"):
        fast.upscale_pil(u8, scale=2)
    with pytest.raises(ValueError, match="expected two positive integers"):
        fast.resize_pil(u8, (0, 4))
    with pytest.raises(ValueError, match="resizes up or not at all"):
        fast.upscale_pil(u8, size=(4, 16))
    with pytest.raises(ValueError, match="resizes up or not at all"):
        fast.upscale_rgb_pil(torch.zeros(3, 8, 8, dtype=torch.uint8), size=(16, 4))
    with pytest.raises(ValueError, match="exactly one of scale and size"):
        fast.upscale_pil(u8)
    fast.channels = 3
    with pytest.raises(ValueError, match="1-channel module"):
        fast.upscale_rgb_pil(torch.zeros(3, 8, 8, dtype=torch.uint8), scale=2)
    import inspect
    for name in ("resize", "resize_image", "upscale", "upscale_image", "upscale_rgb_image", "forward_image"):
        assert "filter" not in inspect.signature(getattr(torch_api.CompiledModule, name)).parameters, name


# ---- 6: the table builder under the sanitizers, stand-alone ----------------------------------------------------------------
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")


@pytest.mark.skipif(not CLANG.exists(), reason="ROCm clang++ not found")
def test_pil_taps_under_asan_ubsan(tmp_path):
    exe = tmp_path / "san_pil_taps"
    subprocess.run([str(CLANG), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                    "-std=c++17", "-ffp-contract=off", "-ffunction-sections", "-fdata-sections", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", f"-I{B.CSRC}", str(B.CSRC / "srcnn_resize_f32.cpp"),
                    str(ROOT / "tests" / "checks" / "san_pil_taps.cpp"), "-Wl,--gc-sections", "-o", str(exe)], check=True)
    env = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
