"""Colour SRCNN models without a GPU: the float64 references against each other, the PyTorch loaders, the blob forms, the
header and exports, the C++ session wrapper and the CLI's blob sizes."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from color_reference import (color_blob, numpy_forward_color, random_color_model, synth_color, torch_forward_color,
                             torch_forward_color_rows)

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("padding", ["replicate", "zero"])
@pytest.mark.parametrize("f2", [1, 3, 5])
def test_torch_reference_matches_numpy_tap_loop(f2, padding):
    model = random_color_model(f2, 11)
    img = synth_color(23, 14, frame=f2)
    a = torch_forward_color(img, model, padding)
    b = numpy_forward_color(img, model, padding)
    assert a.shape == (14, 23, 3)
    assert np.abs(a - b).max() < 1e-9 * max(1.0, np.abs(a).max())


@pytest.mark.parametrize("padding", ["replicate", "zero"])
@pytest.mark.parametrize("f2", [1, 5])
def test_row_window_reference_equals_whole_plane(f2, padding):
    model = random_color_model(f2, 12)
    img = synth_color(31, 40, frame=2)
    whole = torch_forward_color(img, model, padding)
    for r0, r1 in [(0, 5), (3, 17), (20, 40), (39, 40)]:
        assert np.abs(torch_forward_color_rows(img, model, r0, r1, padding) - whole[r0:r1]).max() < 1e-9


class ColorSRCNN(torch.nn.Module):
    def __init__(self, f2, c_in=3, c_out=3, padding_mode="zeros"):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(c_in, 64, 9, padding=4, padding_mode=padding_mode)
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=f2 // 2, padding_mode=padding_mode)
        self.conv3 = torch.nn.Conv2d(32, c_out, 5, padding=2, padding_mode=padding_mode)


@pytest.mark.parametrize("f2", [1, 3, 5])
def test_model_from_state_dict_colour_layout_and_bias_scaling(f2):
    torch.manual_seed(f2)
    net = ColorSRCNN(f2)
    sd = net.state_dict()
    w1, b1, w2, b2, w3, b3 = S.model_from_state_dict(sd, image_order="rgb")
    assert w1.shape == (64, 3, 9, 9) and w2.shape == (32, 64, f2, f2) and w3.shape == (3, 32, 5, 5) and b3.shape == (3,)
    assert all(a.dtype == np.float32 for a in (w1, b1, w2, b2, w3, b3))
    assert np.array_equal(w1, sd["conv1.weight"].numpy()) and np.array_equal(w3, sd["conv3.weight"].numpy())
    assert np.allclose(b1, sd["conv1.bias"].numpy() * 255) and np.allclose(b2, sd["conv2.bias"].numpy() * 255)
    assert np.allclose(b3, sd["conv3.bias"].numpy() * 255)
    _, b1u, _, _, _, b3u = S.model_from_state_dict(sd, input_scale=1.0, image_order="rgb")
    assert np.array_equal(b1u, sd["conv1.bias"].numpy()) and np.array_equal(b3u, sd["conv3.bias"].numpy())


def test_bgr_order_reverses_the_channel_axes_and_computes_the_rgb_model():
    torch.manual_seed(3)
    net = ColorSRCNN(3).double()
    rgb_m = S.model_from_state_dict(net.state_dict(), image_order="rgb")
    bgr_m = S.model_from_state_dict(net.state_dict(), image_order="bgr")
    assert np.array_equal(bgr_m[0], rgb_m[0][:, ::-1]) and np.array_equal(bgr_m[4], rgb_m[4][::-1])
    assert np.array_equal(bgr_m[5], rgb_m[5][::-1]) and np.array_equal(bgr_m[2], rgb_m[2])
    rgb = synth_color(19, 13, frame=1)
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    with torch.no_grad():
        x = torch.from_numpy(np.moveaxis(rgb, 2, 0).astype(np.float64))[None] / 255.0
        ref = np.moveaxis(net.conv3(torch.relu(net.conv2(torch.relu(net.conv1(x)))))[0].numpy(), 0, 2) * 255.0
    got = torch_forward_color(bgr, bgr_m, "zero")
    assert np.abs(got[:, :, ::-1] - ref).max() < 1e-3


def test_model_from_module_colour():
    net = ColorSRCNN(5, padding_mode="replicate")
    model, padding = S.model_from_module(net, image_order="bgr")
    assert padding == "replicate" and model[0].shape == (64, 3, 9, 9)
    with pytest.raises(ValueError, match="image_order"):
        S.model_from_module(net)


def test_missing_image_order_and_mixed_channels_are_rejected():
    sd = ColorSRCNN(3).state_dict()
    with pytest.raises(ValueError, match="image_order"):
        S.model_from_state_dict(sd)
    with pytest.raises(ValueError, match="image_order"):
        S.model_from_state_dict(sd, image_order="yuv")
    for c_in, c_out in [(3, 1), (1, 3)]:
        with pytest.raises(ValueError):
            S.model_from_state_dict(ColorSRCNN(3, c_in, c_out).state_dict(), image_order="rgb")
    # a 1-channel model behaves as before, image_order or not
    one = ColorSRCNN(3, 1, 1).state_dict()
    a, b = S.model_from_state_dict(one), S.model_from_state_dict(one, image_order="bgr")
    assert a[0].shape == (64, 9, 9) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("f2", [1, 3, 5])
def test_split_and_load_model_round_trip_colour_sizes(f2, tmp_path):
    model = random_color_model(f2, 13)
    blob = color_blob(model)
    assert blob.size == {1: 20099, 3: 36483, 5: 69251}[f2] and S.COLOR_MODEL_SIZES[blob.size] == f2
    assert blob.size not in S.MODEL_SIZES
    parts = S.split_model(blob)
    for got, want in zip(parts, model):
        assert np.array_equal(np.asarray(got), np.asarray(want))
    p = tmp_path / "m.f32"
    blob.astype("<f4").tofile(p)
    assert np.array_equal(S.load_model(p), blob)
    with pytest.raises(ValueError):
        S.load_weights(p)


def test_odd_sizes_still_rejected():
    with pytest.raises(ValueError):
        S.split_model(np.zeros(20098, np.float32))
    assert S.MODEL_SIZES == {8129: 1, 24513: 3, 57281: 5}


NEW = ("srcnn_set_model_color", "srcnn_get_model_channels", "srcnn_forward_color", "srcnn_forward_color_dev")


def test_header_declares_and_library_exports_the_colour_entry_points():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srcnn_amd.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in exported and name in S.ABI_SYMBOLS, name


def test_session_set_model_color_compiles(tmp_path):
    src = tmp_path / "s.cpp"
    src.write_text("""
#include "srcnn_amd.hpp"
void use(srcnn::Session &s, const float (*k1)[3][9][9], const float *b1, const float *k2, const float *b2,
         const float (*k3)[32][5][5], const float *b3, const uint8_t *img, uint8_t *out, float *pre)
{
    s.set_model_color(5, k1, b1, k2, b2, k3, b3);
    if (s.model_channels() == 3) s.forward_color(img, 3 * 64, out, 3 * 64, 64, 32, pre, 3 * 64);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT / 'include'}", "-I/opt/rocm/include", str(src)], check=True)


def test_cli_rejects_wrong_length_blobs_and_lists_colour_sizes():
    text = (ROOT / "tools" / "srcnn_cli.cpp").read_text()
    m = re.search(r"if \(n == ([^)]*)\)", text)
    sizes = sorted(int(v) for v in re.findall(r"n == (\d+)", m.group(0)))
    assert sizes == [8129, 20099, 24513, 36483, 57281, 69251]
    for bad in (8128, 20098, 36484, 69252):
        assert bad not in sizes
