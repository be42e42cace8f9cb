"""CPU tests of what stands between the cubic resize's kernels and their LDS arrays, and of the inputs the GPU edge tests
(tests/test_gpu_pipeline_edges.py) rely on.  No device: the product's host code is reached through the tuning build's hooks
srcnn_debug_cubic_table, srcnn_debug_resize_variant and srcnn_debug_resize_limits.

1. the product's coefficient table (compiled by hipcc) equals the oracle's (compiled by the host compiler);
2. resize_variant() sends every shape of pipeline_reference.SHAPES to the kernel written down there by hand;
3. whenever it selects a tiled kernel, the source rows and columns a tile REALLY spans -- taken from the product's own
   tables -- fit the LDS arrays the kernels were compiled with;
4. the numpy restatement of the resize with both vertical passes equals both oracle variants;
5. the tie planes tell the two vertical passes apart on both sides of the column split, from the reference alone.
All of it is integer / bitwise work: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import oracle
import srcnn_cpp_amd as S
from pipeline_reference import (DIRECT, PIPELINE_CASES, SHAPES, TILED, TILED4, chroma_tie_image, discriminating, resize_both,
                                resize_record, split_column, tie_phase, tie_plane, visible_step)

_tuning = None


def tuning_lib():
    global _tuning
    if _tuning is None:
        from srcnn_cpp_amd import build as B
        B.build()
        _tuning = C.CDLL(str(S.tuning_library_path()))
        _tuning.srcnn_debug_cubic_table.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _tuning.srcnn_debug_resize_variant.argtypes = [C.c_int] * 5
        _tuning.srcnn_debug_resize_limits.argtypes = [C.POINTER(C.c_int)]
    return _tuning


def product_table(n_src, n_dst):
    ofs = np.empty(n_dst, np.int32)
    coef = np.empty((n_dst, 4), np.int16)
    assert tuning_lib().srcnn_debug_cubic_table(n_src, n_dst, ofs.ctypes.data, coef.ctypes.data) == 0
    return ofs, coef


def variant(sw, sh, dw, dh, dword_ok):
    return tuning_lib().srcnn_debug_resize_variant(sw, sh, dw, dh, int(dword_ok))


def limits():
    out = (C.c_int * 6)()
    assert tuning_lib().srcnn_debug_resize_limits(out) == 0
    return dict(zip(("RT", "RMAX", "RT4", "RMAX4", "SMAX", "CT"), out))


def test_product_table_equals_the_oracles():
    pairs = [(s, d) for s in range(1, 65) for d in range(1, 257)]
    pairs += [(384, 576), (1920, 3840), (1080, 2160), (640, 832), (3840, 5760)]
    for n_src, n_dst in pairs:
        ofs, coef = product_table(n_src, n_dst)
        o_ofs, o_coef = oracle.cubic_table(n_src, n_dst)
        assert np.array_equal(ofs, o_ofs) and np.array_equal(coef, o_coef), (n_src, n_dst)


def test_limits_hook_reports_the_documented_geometry():
    assert limits() == {"RT": 8, "RMAX": 16, "RT4": 32, "RMAX4": 28, "SMAX": 288, "CT": 256}


@pytest.mark.parametrize("sw,sh,dw,dh,expected,wants_tie", SHAPES)
def test_variant_of_every_table_row(sw, sh, dw, dh, expected, wants_tie):
    assert variant(sw, sh, dw, dh, dw % 4 == 0) == expected
    unaligned = variant(sw, sh, dw, dh, 0)
    assert unaligned in (DIRECT, TILED)                         # no dword stores to an unaligned destination
    if expected != TILED4:
        assert unaligned == expected                            # ... and alignment decides nothing else
    for bad in ((0, sh, dw, dh), (sw, 0, dw, dh), (sw, sh, 0, dh), (sw, sh, dw, -1)):
        assert variant(*bad, 1) < 0
    # the row itself fits the arrays of the kernel it reaches (the sweep below does not hold every row of the table)
    lim = limits()
    if expected != DIRECT:
        rows, cap = (lim["RT4"], lim["RMAX4"]) if expected == TILED4 else (lim["RT"], lim["RMAX"])
        assert true_span(product_table(sh, dh)[0], rows) <= cap
        assert true_span(product_table(sw, dw)[0], lim["CT"]) <= lim["SMAX"]


@pytest.mark.parametrize("w,h,scale,size,fused", PIPELINE_CASES)
def test_pipeline_cases_reach_the_launches_they_are_listed_for(w, h, scale, size, fused):
    """srcnn_process_bgr takes the two fused launches when resize_variant() says tiled4 for dword-aligned rows (the
    context's planes have row stride ow, its output 3 ow): the GPU test's cases, checked here where the hook is."""
    assert oracle.scaled_size(w, h, scale) == size
    ow, oh = size
    assert (variant(w, h, ow, oh, ow % 4 == 0) == TILED4) == fused
    if fused:
        assert ow % 8 == 4
        lim = limits()
        assert true_span(product_table(h, oh)[0], lim["RT4"]) <= lim["RMAX4"]
        assert true_span(product_table(w, ow)[0], lim["CT"]) <= lim["SMAX"]


def true_span(ofs, tile):
    """The most source rows (columns) any tile of `tile` output rows (columns) touches: first tap of its first row to last
    tap of its last, as the kernels compute nrow / ncol from the same table."""
    first = np.arange(0, len(ofs), tile)
    last = np.minimum(first + tile - 1, len(ofs) - 1)
    return int((ofs[last] - ofs[first]).max()) + 4


def test_selected_tiles_fit_their_lds_arrays():
    """sbuf[RMAX4][SMAX] / hbuf[RMAX4][256] (tiled4 and the fused launches) and sbuf[RMAX][SMAX] / hbuf[RMAX][256] (tiled)
    are indexed by the tile's real span; resize_variant()'s ceil() formulas are the only guard.  Rows and columns are
    independent in the selection, so each axis is swept on its own against a partner axis that always qualifies (rows:
    1 -> 1 columns; columns: 1 -> 2 rows).  dword_ok = 1 asks for tiled4, dword_ok = 0 for tiled."""
    lim = limits()
    lib = tuning_lib()
    ofs = np.empty(1400, np.int32)
    coef = np.empty((1400, 4), np.int16)
    worst = {"rows4": 0, "rows": 0, "cols": 0}
    for sh in range(1, 331):
        for dh in range(1, 501):
            t4 = variant(1, sh, 1, dh, 1) == TILED4
            t = variant(1, sh, 1, dh, 0) == TILED
            if not (t4 or t):
                continue
            assert lib.srcnn_debug_cubic_table(sh, dh, ofs.ctypes.data, coef.ctypes.data) == 0
            if t4:
                span = true_span(ofs[:dh], lim["RT4"])
                assert span <= lim["RMAX4"], (sh, dh, span)
                worst["rows4"] = max(worst["rows4"], span)
            if t:
                span = true_span(ofs[:dh], lim["RT"])
                assert span <= lim["RMAX"], (sh, dh, span)
                worst["rows"] = max(worst["rows"], span)
    assert variant(1, 1, 1, 2, 1) == TILED4 and variant(1, 1, 1, 1, 0) == TILED      # the partner axes qualify
    for sw in list(range(1, 41)) + list(range(200, 1301, 7)):
        for dw in list(range(1, 41)) + list(range(250, 1401, 3)):
            t4 = variant(sw, 1, dw, 2, 1) == TILED4
            t = variant(sw, 1, dw, 1, 0) == TILED
            assert t4 == t                                      # one column limit for both
            if not t:
                continue
            assert lib.srcnn_debug_cubic_table(sw, dw, ofs.ctypes.data, coef.ctypes.data) == 0
            span = true_span(ofs[:dw], lim["CT"])
            assert span <= lim["SMAX"], (sw, dw, span)
            worst["cols"] = max(worst["cols"], span)
    print(f"largest real spans among the selected geometries: {worst}, capacities {lim}")
    # the sweep reaches the tiled4 row limit itself: that bound has no slack to lose (the other two, printed above, keep a
    # row resp. a column or two of it)
    assert worst["rows4"] == lim["RMAX4"]


@pytest.mark.parametrize("row", [SHAPES[0], SHAPES[11], SHAPES[12]], ids=lambda r: f"{r[0]}x{r[1]}-{r[2]}x{r[3]}")
def test_numpy_restatement_equals_both_oracle_variants(row):
    sw, sh, dw, dh = row[:4]
    rng = np.random.default_rng(sw + 3 * dh)
    planes = [rng.integers(0, 256, (sh, sw), dtype=np.uint8) for _ in range(3)] + [tie_plane(sw, sh, tie_phase(sh, dh))]
    for src in planes:
        fixed, flt = resize_both(src, dw, dh)
        assert np.array_equal(fixed, oracle.resize_cubic(src, dw, dh, oracle.VERTICAL_FIXED))
        rec = oracle.resize_cubic(src, dw, dh)
        s = split_column(dw)
        assert np.array_equal(flt[:, :s], rec[:, :s]) and np.array_equal(fixed[:, s:], rec[:, s:])
        assert np.array_equal(resize_record(src, dw, dh), rec)


TIE_ROWS = [r for r in SHAPES if r[5]]


@pytest.mark.parametrize("sw,sh,dw,dh,expected,wants_tie", TIE_ROWS)
def test_tie_planes_tell_the_two_passes_apart(sw, sh, dw, dh, expected, wants_tie):
    """What makes the GPU test of the column split a test: on the row's tie plane the passes differ in at least 8 pixels of the
    8 columns below the split and, where the row has a tail, in at least 8 pixels of it; and the picture of record shows the
    step.  A tie row added to the table later must meet this or be dropped (x1.5 with dw % 8 == 1 has no tying tail column)."""
    src = tie_plane(sw, sh, tie_phase(sh, dh))
    below, tail = discriminating(src, dw, dh)
    print(f"{sw}x{sh} -> {dw}x{dh}: fixed != float in {below} pixels below the split, {tail} in the tail")
    assert below >= 8
    if dw % 8:
        assert tail >= 8
        assert visible_step(src, dw, dh) >= 1


def test_every_tie_row_has_a_tail():
    assert len(TIE_ROWS) == 6 and all(r[2] % 8 for r in TIE_ROWS)       # so both sides of the split are held on every one


@pytest.mark.parametrize("w,h,scale,size,fused", [c for c in PIPELINE_CASES if c[2] == 1.5 and c[4]])
def test_pipeline_tie_images_tie_in_the_plane_they_are_meant_to(w, h, scale, size, fused):
    """The grey tie image (B = G = R = tie_plane) ties in Y with flat chroma; the two chroma tie images tie in Cr resp. Cb."""
    ow, oh = size
    grey = np.repeat(tie_plane(w, h, 1)[:, :, None], 3, axis=2)
    y, cr, cb = oracle.bgr2ycrcb(grey)
    assert np.array_equal(y, tie_plane(w, h, 1)) and (cr == 128).all() and (cb == 128).all()
    planes = {"Y": y}
    for comp, name in ((1, "Cr"), (2, "Cb")):
        planes[name] = oracle.bgr2ycrcb(chroma_tie_image(w, h, comp))[comp]
        assert np.array_equal(planes[name], tie_plane(w, h, 1) + 100)
    for name, plane in planes.items():
        below, tail = discriminating(plane, ow, oh)
        assert below >= 8 and tail >= 8, (name, below, tail)
