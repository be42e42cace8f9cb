"""CPU tests of the float32 cubic resize (srcnn_resize_cubic_f32*, torch's bicubic): no device.
1. srcnn_cubic_f32_taps -- the one table builder, also what the kernels run on -- against the float64 restatement;
2. that restatement (tests/resize_f32_reference.py) against torch's own CPU result, which pins it to torch's semantics of A,
   half-pixel centres and index clamping;
3. whenever the selection function chooses the tiled form, the source rows and columns a tile REALLY spans -- taken from the
   product's own tables -- fit the LDS arrays the kernel was compiled with (the tuning build's hooks);
4. the Python binding and the torch front end refuse bad arguments before any call into the library."""
import ctypes as C

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd import torch_api
from resize_f32_reference import ref64, taps64, torch_cpu, uniform

PAIRS = [(1, 5), (3, 7), (4, 8), (33, 49), (250, 511), (300, 900), (29, 13), (300, 7)]
SAME = [1, 2, 7, 64, 333]


@pytest.fixture(scope="module")
def built():
    from srcnn_cpp_amd import build as B
    B.build()                      # hipcc cross-compiles gfx950 without a GPU
    return S.load_library()


@pytest.mark.parametrize("s,n", PAIRS + [(s, s) for s in SAME])
def test_taps_against_the_float64_restatement(built, s, n):
    first, coef = S.cubic_f32_taps(s, n)
    assert first.dtype == np.int32 and coef.dtype == np.float32 and first.shape == (n,) and coef.shape == (n, 4)
    f64, c64 = taps64(s, n)
    assert np.array_equal(first, f64)
    # within 1 float32 ulp of the float64 value (np.spacing of the float32 neighbour; 2^-149 around zero)
    ulp = np.spacing(np.abs(c64).astype(np.float32)).astype(np.float64)
    assert (np.abs(coef.astype(np.float64) - c64) <= ulp).all()
    assert np.abs(coef.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
    if s == n:
        assert np.array_equal(first, np.arange(n))
        assert np.array_equal(coef, np.tile(np.float32([0, 1, 0, 0]), (n, 1)))


def test_taps_refuse_bad_arguments(built):
    first, coef = np.empty(4, np.int32), np.empty((4, 4), np.float32)
    fp, cp = first.ctypes.data_as(C.POINTER(C.c_int)), coef.ctypes.data_as(C.POINTER(C.c_float))
    assert built.srcnn_cubic_f32_taps(0, 4, fp, cp) == S.ERR_INVALID
    assert built.srcnn_cubic_f32_taps(4, -1, fp, cp) == S.ERR_INVALID
    assert built.srcnn_cubic_f32_taps(4, 4, None, cp) == S.ERR_INVALID
    assert built.srcnn_cubic_f32_taps(4, 4, fp, None) == S.ERR_INVALID
    with pytest.raises(ValueError):
        S.cubic_f32_taps(0, 3)
    assert built.srcnn_abi_version() == 1


@pytest.mark.parametrize("sh,sw,dh,dw,bound", [(5, 4, 10, 8, 1e-6), (31, 67, 62, 134, 1e-6),
                                               (17, 33, 25, 49, 1e-4), (64, 250, 97, 511, 1e-4)])
def test_restatement_against_torch_cpu(sh, sw, dh, dw, bound):
    """x2: torch's float32 coordinates are exact, the difference is float32 rounding of the sums (2.4e-7 measured); non-dyadic
    ratios: torch's coordinate error shows (1.5e-5 at 64x250 -> 97x511)."""
    x = uniform((2, sh, sw), sh + dw)
    diff = np.abs(torch_cpu(x, dh, dw).astype(np.float64) - ref64(x, dh, dw)).max()
    print(f"{sh}x{sw} -> {dh}x{dw}: max|torch - ref64| = {diff:.3g}")
    assert diff <= bound


def test_restatement_properties():
    x = uniform((9, 13), 3)
    assert np.array_equal(ref64(x, 9, 13), x.astype(np.float64))             # the same size: an exact copy
    up = ref64(uniform((40, 40), 4), 120, 120)
    assert up.min() < 0.0 and up.max() > 1.0                                  # overshoot is part of the definition: no clamp
    assert np.abs(ref64(np.full((6, 5), 0.3, np.float32), 11, 17) - np.float64(np.float32(0.3))).max() < 1e-15


# ---- the selection function keeps a tile inside its arrays ------------------------------------------------------------------
_tuning = None


def tuning_lib():
    global _tuning
    if _tuning is None:
        from srcnn_cpp_amd import build as B
        B.build()
        _tuning = C.CDLL(str(S.tuning_library_path()))
        _tuning.srcnn_debug_resize_f32_variant.argtypes = [C.c_int] * 4
        _tuning.srcnn_debug_resize_f32_limits.argtypes = [C.POINTER(C.c_int)]
    return _tuning


def limits():
    out = (C.c_int * 4)()
    assert tuning_lib().srcnn_debug_resize_f32_limits(out) == 0
    return dict(zip(("RT", "RMAX", "SMAX", "CT"), out))


def true_span(first, tile):
    """The most source samples any tile of `tile` outputs touches, as the kernel computes nrow / ncol from the same table."""
    lo = np.arange(0, len(first), tile)
    hi = np.minimum(lo + tile - 1, len(first) - 1)
    return int((first[hi] - first[lo]).max()) + 4


def test_limits_hook_reports_the_documented_geometry():
    assert limits() == {"RT": 16, "RMAX": 20, "SMAX": 264, "CT": 256}


def test_selected_tiles_fit_their_lds_arrays(built):
    """sbuf[F32_RMAX][F32_SMAX] and hbuf[F32_RMAX][256] are indexed by the tile's real span; resize_f32_variant()'s ceil()
    formulas are the only guard.  Rows and columns are independent in the selection, so each axis is swept on its own against
    a partner axis that always qualifies (1 -> 1)."""
    lim, lib = limits(), tuning_lib()
    variant = lib.srcnn_debug_resize_f32_variant
    assert variant(1, 1, 1, 1) == 1
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)):
        assert variant(*bad) < 0
    worst = {"rows": 0, "cols": 0}
    tiled = 0
    for s in list(range(1, 131)) + [250, 300, 540, 1080]:
        for n in list(range(1, 301)) + [511, 900, 1080, 2160]:
            if variant(1, s, 1, n) == 1:
                tiled += 1
                worst["rows"] = max(worst["rows"], true_span(S.cubic_f32_taps(s, n)[0], lim["RT"]))
    for s in list(range(1, 41)) + list(range(200, 1301, 7)) + [960, 1920]:
        for n in list(range(1, 41)) + list(range(250, 1401, 3)) + [1920, 3840]:
            if variant(s, 1, n, 1) == 1:
                tiled += 1
                worst["cols"] = max(worst["cols"], true_span(S.cubic_f32_taps(s, n)[0], lim["CT"]))
    print(f"largest real spans among {tiled} tiled geometries: {worst}, capacities {lim}")
    assert tiled > 1000 and worst["rows"] <= lim["RMAX"] and worst["cols"] <= lim["SMAX"]
    # the same size and every up-scale are tiled; down-scaling below the span bound is not
    assert variant(1920, 1080, 3840, 2160) == 1 and variant(300, 200, 300, 200) == 1
    assert variant(300, 200, 7, 9) == 0 and variant(29, 23, 13, 11) == 0


# ---- refusals in Python, before any call into the library ------------------------------------------------------------------
class _NoCall:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C ABI with bad arguments")


def _shell_context():
    ctx = object.__new__(S.Context)           # no device needed: only the Python-side validation runs
    ctx._lib, ctx._h = _NoCall(), None
    return ctx


def test_python_binding_refuses_before_the_library():
    ctx = _shell_context()
    good = np.zeros((3, 8, 8), np.float32)
    for call in (ctx.resize_cubic_f32, ctx.process_f32):
        with pytest.raises(TypeError):
            call(good.astype(np.float64), 16, 16)                    # wrong dtype
        with pytest.raises(TypeError):
            call(np.zeros((8, 8), np.uint8), 16, 16)
        with pytest.raises(TypeError):
            call(np.zeros(8, np.float32), 16, 16)                    # wrong rank
        with pytest.raises(TypeError):
            call(np.zeros((1, 3, 8, 8), np.float32), 16, 16)
        with pytest.raises(TypeError):
            call([[0.0]], 16, 16)                                    # not an array
        with pytest.raises(ValueError):
            call(np.zeros((3, 8, 16), np.float32)[:, :, ::2], 16, 16)        # rows not contiguous
        with pytest.raises(ValueError):
            call(np.zeros((3, 0, 8), np.float32), 16, 16)            # empty
        for bad in ((0, 16), (16, -1), (16.0, 16), (True, 16)):
            with pytest.raises(ValueError):
                call(good, *bad)


def test_torch_front_end_refuses_before_the_library():
    fast = object.__new__(torch_api.CompiledModule)
    fast.ctx, fast.channels, fast.device, fast._side = _NoCall(), 1, 0, None
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError, match="exactly one"):
        fast.upscale(x)                                              # neither
    with pytest.raises(ValueError, match="exactly one"):
        fast.upscale(x, scale=2, size=(16, 16))                      # both
    for call in (lambda t: fast.upscale(t, size=(16, 16)), lambda t: fast.upscale(t, scale=2), lambda t: fast.resize(t, (16, 16))):
        with pytest.raises(ValueError):
            call(x.double())                                         # wrong dtype
        with pytest.raises(ValueError):
            call(torch.zeros(8, 8))                                  # wrong rank
        with pytest.raises(ValueError):
            call(torch.zeros(1, 3, 8, 8))                            # wrong channel count
        with pytest.raises(ValueError):
            call(x)                                                  # a CPU tensor: there is no CPU path
    for bad in ((16,), (0, 16), (16, 2.5), None, 16):
        with pytest.raises(ValueError):
            torch_api.check_size(bad)
    assert torch_api.check_size((5, 7)) == (5, 7) and torch_api.check_size([np.int64(5), 7]) == (5, 7)
