"""Models of other widths (srcnn_set_model_shape, srcnn_get_model_shape) without a GPU: the ABI, the loaders' acceptance and
refusals, what Context.set_model hands to the library (on a context without a device), the references' own consistency, and
the device code of the wide forms of layers 2 and 3."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd import build as B
import spatial_listing as L
from color_reference import random_color_model, torch_forward_color
from spatial_reference import band_seams as band_seams_64_32
from spatial_reference import random_model, torch_forward
from wide_reference import as_plain, band_seams, embed, forward, forward_rows, padded_widths, random_wide_model

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["srcnn_set_model_shape", "srcnn_get_model_shape"]
UNIT = "srcnn_wide_kernels.hip"


@pytest.fixture(scope="module")
def lib():
    B.build()
    return S.load_library()


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_shape_entry_points(lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srcnn_amd.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in srcnn_amd.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in S.ABI_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    assert set(NEW_SYMBOLS) <= {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert lib.srcnn_abi_version() == 1                      # a plain addition: no version bump


def test_null_context(lib):
    assert lib.srcnn_set_model_shape(None, 1, 128, 3, 64, None, None, None, None, None, None) == S.ERR_INVALID
    assert lib.srcnn_get_model_shape(None, None, None, None, None) == S.ERR_INVALID


def test_header_says_what_the_padding_does():
    text = " ".join((ROOT / "include" / "srcnn_amd.h").read_text().split())
    assert "zero weights and zero biases" in text and "is 0 after its ReLU" in text
    assert "64 * ceil(n1 / 64)" in text and "32 * ceil(n2 / 32)" in text


# ---- the loaders ----------------------------------------------------------------------------------------------------------
class Net(torch.nn.Module):
    def __init__(self, channels, n1, f2, n2, padding_mode="zeros", conv2_in=None):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(channels, n1, 9, padding=4, padding_mode=padding_mode)
        self.conv2 = torch.nn.Conv2d(n1 if conv2_in is None else conv2_in, n2, f2, padding=f2 // 2, padding_mode=padding_mode)
        self.conv3 = torch.nn.Conv2d(n2, channels, 5, padding=2, padding_mode=padding_mode)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n1,n2", [(128, 64), (96, 48), (32, 16)])
def test_loaders_accept_other_widths(channels, n1, n2):
    torch.manual_seed(n1 + channels)
    net = Net(channels, n1, 3, n2)
    sd = net.state_dict()
    order = "rgb" if channels == 3 else None
    model = S.model_from_state_dict(sd, input_scale=1.0, image_order=order)
    (w1, b1, w2, b2, w3, b3), padding = S.model_from_module(net, input_scale=1.0, image_order=order)
    assert padding == "zero"
    for got, want in zip(model, (w1, b1, w2, b2, w3, b3)):
        assert np.array_equal(got, want)
    assert w1.shape == (n1, channels, 9, 9) and w2.shape == (n2, n1, 3, 3) and w3.shape == (channels, n2, 5, 5)
    assert b1.shape == (n1,) and b2.shape == (n2,) and b3.shape == (channels,)
    assert all(a.dtype == np.float32 for a in (w1, b1, w2, b2, w3, b3))
    assert np.array_equal(w2, sd["conv2.weight"].numpy()) and np.array_equal(w1, sd["conv1.weight"].numpy())
    # the biases carry the input scale, as for 64 / 32
    scaled = S.model_from_state_dict(sd, input_scale=255.0, image_order=order)
    assert np.array_equal(scaled[1], (sd["conv1.bias"].double().numpy() * 255.0).astype(np.float32))
    assert np.array_equal(scaled[5], (sd["conv3.bias"].double().numpy() * 255.0).astype(np.float32))
    if channels == 3:
        bgr = S.model_from_state_dict(sd, input_scale=1.0, image_order="bgr")
        assert np.array_equal(bgr[0], w1[:, ::-1]) and np.array_equal(bgr[4], w3[::-1]) and np.array_equal(bgr[5], b3[::-1])
        with pytest.raises(ValueError):
            S.model_from_state_dict(sd, input_scale=1.0)          # a 3-channel model needs image_order, whatever its widths


def test_loaders_keep_the_64_32_forms():
    sd = Net(1, 64, 3, 32).state_dict()
    w1, b1, w2, b2, w3, b3 = S.model_from_state_dict(sd)
    assert w1.shape == (64, 9, 9) and w2.shape == (32, 64, 3, 3) and w3.shape == (32, 5, 5) and isinstance(b3, float)


@pytest.mark.parametrize("n1,n2,conv2_in", [(129, 64, None), (128, 65, None), (128, 64, 127), (64, 32, 63)])
def test_loaders_reject_widths_out_of_range(n1, n2, conv2_in):
    net = Net(1, n1, 3, n2, conv2_in=conv2_in)
    with pytest.raises(ValueError):
        S.model_from_state_dict(net.state_dict())
    with pytest.raises(ValueError):
        S.model_from_module(net)


def test_loaders_reject_no_filters_and_keep_their_other_refusals():
    sd = {k: v.clone() for k, v in Net(1, 128, 3, 64).state_dict().items()}
    empty = dict(sd)
    empty["conv1.weight"], empty["conv1.bias"], empty["conv2.weight"] = torch.zeros(0, 1, 9, 9), torch.zeros(0), torch.zeros(64, 0, 3, 3)
    with pytest.raises(ValueError):
        S.model_from_state_dict(empty)                         # n1 = 0
    bad = dict(sd)
    bad["conv2.weight"] = torch.zeros(64, 128, 7, 7)
    with pytest.raises(ValueError):
        S.model_from_state_dict(bad)                           # f2 = 7
    bad = dict(sd)
    bad["conv1.weight"] = torch.zeros(128, 1, 7, 7)
    with pytest.raises(ValueError):
        S.model_from_state_dict(bad)                           # f1 = 7
    bad = dict(sd)
    bad["conv3.weight"], bad["conv3.bias"] = torch.zeros(3, 64, 5, 5), torch.zeros(3)
    with pytest.raises(ValueError):
        S.model_from_state_dict(bad, image_order="rgb")        # 1 channel in, 3 out
    with pytest.raises(ValueError):
        S.model_from_module(Net(1, 128, 3, 64, padding_mode="reflect"))


# ---- Context.set_model on a context without a device ----------------------------------------------------------------------
class _Recorder:
    """Stands in for the library: records srcnn_set_model_shape's arguments, refuses everything else."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == "srcnn_set_model_shape":
            return lambda h, *a: self.calls.append(a) or 0
        raise AssertionError(f"{name} reached the C ABI")


def _shell_context():
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = _Recorder(), None
    return ctx


@pytest.mark.parametrize("channels,n1,f2,n2", [(1, 128, 3, 64), (3, 128, 5, 64), (1, 96, 1, 48), (3, 32, 3, 16), (1, 64, 3, 64),
                                               (1, 128, 1, 32), (1, 1, 1, 1)])
def test_set_model_reads_the_widths_from_the_shapes(channels, n1, f2, n2):
    ctx = _shell_context()
    ctx.set_model(*random_wide_model(channels, n1, f2, n2, 1))
    (ch, a, f, b, *_), = ctx._lib.calls
    assert (ch, a, f, b) == (channels, n1, f2, n2)
    if channels == 1:           # the squeezed 1-channel shapes and a (n2, n1) layer 2 are read the same way
        w1, b1, w2, b2, w3, b3 = random_wide_model(1, n1, f2, n2, 1)
        ctx.set_model(w1[:, 0], b1, w2[:, :, 0, 0] if f2 == 1 else w2, b2, w3[0], float(b3[0]))
        assert ctx._lib.calls[1][:4] == (1, n1, f2, n2)


def test_set_model_rejects_bad_shapes_before_the_library():
    good = random_wide_model(1, 128, 3, 64, 1)
    for n1, n2 in [(129, 64), (128, 65)]:
        w1, b1, w2, b2, w3, b3 = (np.zeros(s, np.float32) for s in [(n1, 1, 9, 9), (n1,), (n2, n1, 3, 3), (n2,), (1, n2, 5, 5), (1,)])
        with pytest.raises(ValueError):
            _shell_context().set_model(w1, b1, w2, b2, w3, b3)
    w1, b1, w2, b2, w3, b3 = good
    for bad in [(w1[:127], b1, w2, b2, w3, b3),                 # w2's second dimension differs from conv1's output count
                (w1, b1, np.zeros((64, 128, 7, 7), np.float32), b2, w3, b3), (w1, b1, w2, b2, w3[:, :63], b3),
                (w1, b1[:100], w2, b2, w3, b3), (w1, b1, w2, b2, w3, np.zeros(3, np.float32)),
                (np.zeros((128, 2, 9, 9), np.float32), b1, w2, b2, w3, b3)]:
        ctx = _shell_context()
        with pytest.raises(ValueError):
            ctx.set_model(*bad)
        assert not ctx._lib.calls


def test_flat_arrays_keep_meaning_64_32():
    class Plain(_Recorder):
        def __getattr__(self, name):
            if name == "srcnn_set_model":
                return lambda h, *a: self.calls.append(("set_model", a[0])) or 0
            return super().__getattr__(name)
    ctx = object.__new__(S.Context)
    ctx._lib, ctx._h = Plain(), None
    w1, b1, w2, b2, w3, b3 = random_model(3, 1)
    ctx.set_model(w1, b1, w2, b2, w3, b3)
    assert ctx._lib.calls == [("set_model", 3)]


# ---- the references -------------------------------------------------------------------------------------------------------
def test_reference_restates_the_existing_ones_at_64_32():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (23, 31)).astype(np.float64)
    m = random_model(3, 1)
    wide = (m[0][:, None], m[1], m[2], m[3], m[4][None], np.array([m[5]], np.float32))
    assert np.array_equal(forward(y[None], wide)[0], torch_forward(y, m))
    assert as_plain(wide)[0].shape == (64, 9, 9) and as_plain(wide)[5] == m[5]
    img = rng.integers(0, 256, (23, 31, 3)).astype(np.float64)
    cm = random_color_model(5, 1)
    for padding in ("replicate", "zero"):
        assert np.array_equal(np.moveaxis(forward(np.moveaxis(img, 2, 0), cm, padding), 0, 2), torch_forward_color(img, cm, padding))


@pytest.mark.parametrize("padding", ["replicate", "zero"])
def test_row_windows_and_embedding_of_the_reference(padding):
    model = random_wide_model(3, 100, 3, 40, 2)
    x = np.random.default_rng(1).uniform(0, 255, (3, 40, 21))
    ref = forward(x, model, padding)
    for r0, r1 in [(0, 7), (11, 25), (33, 40)]:
        assert np.allclose(forward_rows(x, model, r0, r1, padding), ref[:, r0:r1], rtol=0, atol=1e-9)
    assert np.allclose(forward(x, embed(model, 128, 64), padding), ref, rtol=0, atol=1e-9)     # zero channels add zeros
    assert 0.2 < np.abs(ref - 60).mean() / np.abs(forward(x, random_wide_model(3, 64, 3, 32, 2), padding) - 60).mean() < 5


def test_band_seams_formula():
    assert padded_widths(128, 64) == (128, 64) and padded_widths(96, 48) == (128, 64) and padded_widths(32, 16) == (64, 32)
    assert padded_widths(65, 32) == (128, 32) and padded_widths(64, 33) == (64, 64) and padded_widths(1, 1) == (64, 32)
    for w, h, f2 in [(3840, 2160, 5), (3840, 2160, 1), (1920, 1080, 3), (1024, 768, 3), (7680, 4320, 5)]:
        assert band_seams(w, h, f2, 64, 32) == band_seams_64_32(w, h, f2) == band_seams(w, h, f2, 32, 16)
    # 768 B per pixel of a 1024 x 768 plane exceed 512 MiB: two bands; 1024 x 640 is one
    assert band_seams(1024, 768, 3, 128, 64) == [384] and band_seams(1024, 768, 5, 128, 64) == [384]
    assert band_seams(1024, 640, 5, 128, 64) == []
    assert len(band_seams(3840, 2160, 5, 128, 64)) > len(band_seams_64_32(3840, 2160, 5))


# ---- the device code of the wide forms (srcnn_spatial_kernels.hip) -----------------------------------------------------------
def test_the_unit_is_gone_from_the_build_and_from_disk():
    assert UNIT not in [u[0] for u in B.UNITS] and not (B.CSRC / UNIT).exists()


def test_the_units_kernels():
    l2, l3 = L.kernels(L.L2_WIDE), L.kernels(L.L3_WIDE)
    ks = l2 + l3
    assert len(l2) == 6 and len(l3) == 12 and len(ks) == 18
    assert len({k[0] for k in ks}) == 18
    assert sorted(re.search(L.L2_WIDE, k[0]).groups() for k in l2) == sorted((f2, z) for f2 in "135" for z in "01")
    # layer 3: C = 1, 3 x replicate, zero x {bytes, bytes + pre-clamp, floats}
    forms = sorted(re.search(L.L3_WIDE, k[0]).groups() for k in l3)
    assert forms == sorted((c, pre, z, t) for c in "13" for z in "01" for pre, t in (("0", "h"), ("1", "h"), ("0", "f")))
    for name, desc, body in ks:
        assert L.private_bytes(desc) == 0, f"{name} has a private segment"
        assert "scratch_" not in body, name
        assert L.mfma_kinds(body) == {"v_mfma_f32_32x32x2_f32"}, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 512
    for name, desc, body in l3:     # the LDS row of the strip: 2 x C x 5 x 128 floats, nothing else
        c = int(re.search(L.L3_WIDE, name).group(1))
        assert L.static_lds_bytes(desc) == 2 * c * 5 * 128 * 4
