"""9-3-5 / 9-5-5 models (srcnn_set_model) without a GPU: blob sizes, the PyTorch state-dict mapping, the float64
restatement the GPU tests use as their yardstick, and the CLI's refusal of a blob of any other size."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from spatial_reference import model_blob, numpy_forward, random_model, torch_forward, torch_forward_rows

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("f2", [1, 3, 5])
def test_split_model_round_trip(f2, tmp_path):
    model = random_model(f2, 0)
    blob = model_blob(model)
    assert blob.size == {1: 8129, 3: 24513, 5: 57281}[f2]
    assert S.MODEL_SIZES[blob.size] == f2
    for got, want in zip(S.split_model(blob), model):
        assert np.array_equal(np.asarray(got), np.asarray(want, np.float32))
    p = tmp_path / "m.f32"
    blob.tofile(p)
    assert np.array_equal(S.load_model(p), blob)


def test_split_model_of_the_shipped_blob_is_split_weights():
    blob = S.load_weights()
    for a, b in zip(S.split_model(blob), S.split_weights(blob)):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("n", [0, 1, 8128, 8130, 16384, 24512, 24514, 40897, 57280, 57282, 2 * 8129])
def test_other_blob_sizes_are_rejected(n, tmp_path):
    blob = np.zeros(n, np.float32)
    with pytest.raises(ValueError):
        S.split_model(blob)
    p = tmp_path / "bad.f32"
    blob.tofile(p)
    with pytest.raises(ValueError):
        S.load_model(p)


@pytest.mark.parametrize("n", [24513, 57281])
def test_load_and_split_weights_still_take_only_the_9_1_5_blob(n, tmp_path):
    p = tmp_path / "m.f32"
    np.zeros(n, np.float32).tofile(p)
    with pytest.raises(ValueError):
        S.load_weights(p)


class _Srcnn(torch.nn.Module):
    def __init__(self, f2):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(1, 64, 9, padding=4)
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=(f2 - 1) // 2)
        self.conv3 = torch.nn.Conv2d(32, 1, 5, padding=2)


@pytest.mark.parametrize("f2", [1, 3, 5])
def test_model_from_state_dict_layout_and_bias_scaling(f2):
    torch.manual_seed(f2)
    net = _Srcnn(f2)
    sd = net.state_dict()
    w1, b1, w2, b2, w3, b3 = S.model_from_state_dict(sd, input_scale=255.0)
    assert w1.shape == (64, 9, 9) and w1.dtype == np.float32
    assert w2.shape == ((32, 64) if f2 == 1 else (32, 64, f2, f2))
    assert w3.shape == (32, 5, 5) and isinstance(b3, float)
    assert np.array_equal(w1, sd["conv1.weight"].numpy()[:, 0])
    assert np.array_equal(w2.reshape(32, 64, f2, f2), sd["conv2.weight"].numpy())
    assert np.array_equal(w3, sd["conv3.weight"].numpy()[0])
    assert np.allclose(b1, sd["conv1.bias"].numpy() * 255.0, rtol=1e-6)
    assert np.allclose(b2, sd["conv2.bias"].numpy() * 255.0, rtol=1e-6)
    assert b3 == pytest.approx(float(sd["conv3.bias"][0]) * 255.0, rel=1e-6)
    u = S.model_from_state_dict(sd, input_scale=1.0)
    assert np.array_equal(u[1], sd["conv1.bias"].numpy())
    # the scaled model on 0..255 is 255 x the [0, 1] model (ReLU is positively homogeneous): away from the borders, where
    # replicate and zero padding agree, it equals the PyTorch module with zero padding
    rng = np.random.default_rng(f2)
    y = rng.integers(0, 256, (40, 44)).astype(np.uint8)
    with torch.no_grad():
        x = torch.from_numpy(y.astype(np.float64) / 255.0)[None, None]
        net = net.double()
        z = net.conv3(torch.relu(net.conv2(torch.relu(net.conv1(x)))))[0, 0].numpy() * 255.0
    m = torch_forward(y, S.model_from_state_dict(sd))
    r = 6 + (f2 - 1) // 2
    assert np.abs(m[r:-r, r:-r] - z[r:-r, r:-r]).max() < 1e-3


def test_model_from_state_dict_rejects_bad_shapes():
    sd = _Srcnn(3).state_dict()
    bad = dict(sd)
    bad["conv2.weight"] = torch.zeros(32, 64, 7, 7)
    with pytest.raises(ValueError):
        S.model_from_state_dict(bad)
    bad = dict(sd)
    bad["conv1.weight"] = torch.zeros(64, 1, 7, 7)
    with pytest.raises(ValueError):
        S.model_from_state_dict(bad)
    bad = dict(sd)
    del bad["conv3.bias"]
    with pytest.raises(KeyError):
        S.model_from_state_dict(bad)


@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("w,h", [(11, 7), (7, 11), (1, 1), (3, 2)])
def test_torch_restatement_matches_numpy_loop(f2, w, h):
    """Pins orientation (cross-correlation) and the per-layer replicate padding of the yardstick on tiny images."""
    rng = np.random.default_rng(w * 100 + h)
    y = rng.integers(0, 256, (h, w)).astype(np.uint8)
    model = random_model(f2, 3)
    a, b = torch_forward(y, model), numpy_forward(y, model)
    assert np.abs(a - b).max() < 1e-9


def test_asymmetric_tap_orientation():
    """A one-hot off-centre layer-2 tap (kh, kw) = (0, 3) shifts the layer-1 map: output(y, x) reads (y - 2, x + 1)."""
    model = list(random_model(5, 1))
    w2 = np.zeros((32, 64, 5, 5), np.float32)
    w2[:, :, 0, 3] = random_model(1, 1)[2]
    model[2] = w2
    y = np.random.default_rng(9).integers(0, 256, (11, 7)).astype(np.uint8)
    base = list(model)
    base[2] = w2[:, :, 0, 3]
    from spatial_reference import torch_layer3, torch_layers12
    m1 = torch_layers12(y, base).numpy()
    ys = np.clip(np.arange(11) - 2, 0, 10)[:, None]
    xs = np.clip(np.arange(7) + 1, 0, 6)[None, :]
    want = torch_layer3(m1[:, ys, xs], model)
    assert np.abs(numpy_forward(y, model) - want).max() < 1e-9


def test_row_windows_equal_the_whole_plane():
    y = np.random.default_rng(4).integers(0, 256, (60, 23)).astype(np.uint8)
    model = random_model(5, 2)
    full = torch_forward(y, model)
    for r0, r1 in [(0, 5), (10, 30), (52, 60), (0, 60)]:
        assert np.abs(torch_forward_rows(y, model, r0, r1) - full[r0:r1]).max() < 1e-9


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from srcnn_cpp_amd import build as B
    B.build()
    exe = tmp_path_factory.mktemp("cli_model") / "srcnn_amd"
    subprocess.run(["g++", "-std=c++17", "-O2", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tools'}",
                    str(ROOT / "tools" / "srcnn_cli.cpp"), f"-L{ROOT / 'srcnn_cpp_amd'}", "-lsrcnn_amd", "-lz", "-ldl",
                    f"-Wl,-rpath,{ROOT / 'srcnn_cpp_amd'}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("n", [100, 8128, 8130, 24512, 57280, 57282])
def test_cli_rejects_a_wrong_length_weights_blob(cli, tmp_path, n):
    from PIL import Image
    img = tmp_path / "a.ppm"
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(img)
    w = tmp_path / "w.f32"
    np.zeros(n, np.float32).tofile(w)
    r = subprocess.run([str(cli), f"--weights={w}", str(img), str(tmp_path / "b.ppm")], capture_output=True, text=True)
    assert r.returncode == 255 and "model load failure" in r.stdout
    assert not (tmp_path / "b.ppm").exists()
