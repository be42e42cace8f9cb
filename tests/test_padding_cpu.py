"""Zero padding (srcnn_set_padding) without a GPU: the float64 zero-pad reference the GPU tests use as their yardstick against
an independent numpy loop, model_from_module's reading of a PyTorch SRCNN, the ABI and C++ surface, and the CLI's refusals."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import srcnn_cpp_amd as S
from srcnn_cpp_amd.synth import synth_luma
from spatial_reference import random_model, torch_forward
from zero_pad_reference import numpy_forward_zero, torch_forward_zero, torch_forward_zero_rows

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("w,h", [(1, 1), (3, 3), (9, 5), (17, 4), (23, 19)])
def test_zero_reference_matches_numpy_tap_loop(f2, w, h):
    model = random_model(f2, 1)
    y = synth_luma(w, h, frame=2)
    ref = torch_forward_zero(y, model)
    assert ref.shape == (h, w)
    assert np.abs(ref - numpy_forward_zero(y, model)).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def test_zero_and_replicate_differ_at_the_border_only():
    model = random_model(5, 2)
    y = synth_luma(40, 37, frame=1)
    d = np.abs(torch_forward_zero(y, model) - torch_forward(y, model)) > 1e-9
    reach = 6 + 2
    assert d[:reach].any() and d[-reach:].any() and d[:, :reach].any() and d[:, -reach:].any()
    assert not d[reach:-reach, reach:-reach].any()


@pytest.mark.parametrize("f2", [1, 5])
def test_zero_row_windows_equal_the_whole_plane(f2):
    model = random_model(f2, 3)
    y = synth_luma(31, 90, frame=4)
    full = torch_forward_zero(y, model)
    for r0, r1 in [(0, 7), (3, 20), (40, 51), (80, 90), (0, 90)]:
        assert np.abs(torch_forward_zero_rows(y, model, r0, r1) - full[r0:r1]).max() <= 1e-9 * np.abs(full).max()


class _Srcnn(torch.nn.Module):
    def __init__(self, f2, modes=("zeros",) * 3, pads=None):
        super().__init__()
        pads = pads or (4, (f2 - 1) // 2, 2)
        self.conv1 = torch.nn.Conv2d(1, 64, 9, padding=pads[0], padding_mode=modes[0])
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=pads[1], padding_mode=modes[1])
        self.conv3 = torch.nn.Conv2d(32, 1, 5, padding=pads[2], padding_mode=modes[2])


@pytest.mark.parametrize("f2", [1, 3, 5])
@pytest.mark.parametrize("scale", [255.0, 1.0])
def test_model_from_module_maps_weights_and_scales_biases(f2, scale):
    torch.manual_seed(f2)
    m = _Srcnn(f2)
    model, padding = S.model_from_module(m, input_scale=scale)
    assert padding == "zero"
    w1, b1, w2, b2, w3, b3 = model
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    assert np.array_equal(w1, sd["conv1.weight"].reshape(64, 9, 9))
    assert np.allclose(b1, sd["conv1.bias"] * scale, rtol=1e-6)
    assert np.array_equal(w2, sd["conv2.weight"] if f2 > 1 else sd["conv2.weight"].reshape(32, 64))
    assert np.allclose(b2, sd["conv2.bias"] * scale, rtol=1e-6)
    assert np.array_equal(w3, sd["conv3.weight"].reshape(32, 5, 5))
    assert b3 == pytest.approx(float(sd["conv3.bias"][0]) * scale, rel=1e-6)


def test_model_from_module_reads_replicate_and_same():
    assert S.model_from_module(_Srcnn(5, modes=("replicate",) * 3))[1] == "replicate"
    assert S.model_from_module(_Srcnn(3, pads=("same", "same", "same")))[1] == "zero"


@pytest.mark.parametrize("kwargs", [
    dict(pads=(0, 0, 0)),                                   # unpadded
    dict(pads=("valid", 1, 2)),
    dict(pads=(4, 0, 2)),                                   # one layer unpadded
    dict(modes=("reflect",) * 3),
    dict(modes=("zeros", "circular", "zeros")),
    dict(modes=("zeros", "replicate", "zeros")),            # mixed
])
def test_model_from_module_rejects_other_padding(kwargs):
    with pytest.raises(ValueError):
        S.model_from_module(_Srcnn(3, **kwargs))


def test_model_from_module_needs_three_convs():
    m = torch.nn.Module()
    m.conv1 = torch.nn.Conv2d(1, 64, 9, padding=4)
    with pytest.raises(ValueError):
        S.model_from_module(m)


def test_header_and_library_carry_the_padding_api():
    text = (ROOT / "include" / "srcnn_amd.h").read_text()
    assert re.search(r"SRCNN_PAD_REPLICATE\s*=\s*0", text) and re.search(r"SRCNN_PAD_ZERO\s*=\s*1", text)
    assert re.search(r"int srcnn_set_padding\(srcnn_ctx \*ctx, int padding\);", text)
    assert re.search(r"int srcnn_get_padding\(const srcnn_ctx \*ctx\);", text)
    assert {"srcnn_set_padding", "srcnn_get_padding"} <= set(S.ABI_SYMBOLS)
    assert (S.PAD_REPLICATE, S.PAD_ZERO) == (0, 1)
    lib = S.load_library()
    assert lib.srcnn_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.library_path())], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T srcnn_set_padding$", out, re.M) and re.search(r" T srcnn_get_padding$", out, re.M)
    assert lib.srcnn_set_padding(None, 1) == S.ERR_INVALID
    assert lib.srcnn_get_padding(None) == S.ERR_INVALID


def test_session_set_padding_compiles(tmp_path):
    src = tmp_path / "pad.cpp"
    src.write_text("#include <srcnn_amd.hpp>\n"
                   "int use(srcnn::Session &s) { s.set_padding(SRCNN_PAD_ZERO); const srcnn::Session &c = s;\n"
                   "  return c.padding() == SRCNN_PAD_ZERO ? 0 : srcnn_get_padding(nullptr); }\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src)], check=True)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from srcnn_cpp_amd import build as B
    B.build()
    exe = tmp_path_factory.mktemp("cli") / "srcnn_amd"
    subprocess.run(["g++", "-std=c++17", "-O2", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tools'}",
                    str(ROOT / "tools" / "srcnn_cli.cpp"), f"-L{ROOT / 'srcnn_cpp_amd'}", "-lsrcnn_amd", "-lz", "-ldl",
                    f"-Wl,-rpath,{ROOT / 'srcnn_cpp_amd'}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    return exe


def _image(tmp_path):
    from PIL import Image
    p = tmp_path / "a.ppm"
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(p)
    return p


def test_cli_rejects_a_bogus_padding_before_the_gpu(cli, tmp_path):
    r = subprocess.run([str(cli), "--padding=bogus", str(_image(tmp_path))], capture_output=True, text=True)
    assert r.returncode != 0 and "--padding=bogus" in r.stdout and "GPU" not in r.stdout
    assert "--padding=zero|replicate" in subprocess.run([str(cli)], capture_output=True, text=True).stdout


def test_cli_refuses_zero_padding_with_refbytes(cli, tmp_path):
    r = subprocess.run([str(cli), "--padding=zero", "--refbytes", str(_image(tmp_path))], capture_output=True, text=True)
    assert r.returncode != 0 and "--refbytes" in r.stdout and "GPU" not in r.stdout
