"""Command-line tool (tools/srcnn_cli.cpp): the
reference tool's argument rules and exit codes (src/srcnn.cpp:331-447, :707-731),
own PNG/PPM codecs.  CPU tests cover parsing, codecs and every exit that comes
before the GPU is touched; the GPU tests run the whole tool, one picture per
process, against the oracle (the reference's published example, scales from 3.0
down to 0.3, both byte modes) and against float64 restatements of the models
that --weights= / $SRCNN_WEIGHTS load (tests/cli_reference.py)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from srcnn_cpp_amd import build as B
    B.build()
    exe = tmp_path_factory.mktemp("cli") / "srcnn_amd"
    subprocess.run(["g++", "-std=c++17", "-O2", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tools'}",
                    str(ROOT / "tools" / "srcnn_cli.cpp"), f"-L{ROOT / 'srcnn_cpp_amd'}", "-lsrcnn_amd", "-lz", "-ldl",
                    f"-Wl,-rpath,{ROOT / 'srcnn_cpp_amd'}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True, timeout=600)
    return exe


def run(exe, *args, cwd=None, env=None):
    """One process of the tool; $SRCNN_WEIGHTS of the caller's environment never reaches it, `env` adds variables."""
    e = {k: v for k, v in os.environ.items() if k != "SRCNN_WEIGHTS"}
    e.update({k: str(v) for k, v in (env or {}).items()})
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, cwd=cwd, env=e, timeout=120)


def test_no_arguments_prints_title_and_help(cli):
    r = run(cli)                                            # src/srcnn.cpp:709-715: returns 0
    assert r.returncode == 0
    assert "Super-Resolution with deep Convolutional Neural Networks" in r.stdout
    assert "--scale=( ratio: 0.1 to .. )" in r.stdout and "--noverbose" in r.stdout
    assert run(cli, "--help", "x.png").returncode == 0      # --help wins over a source (:394)


def test_load_failure_exit_code(cli, tmp_path):
    r = run(cli, tmp_path / "missing.png")
    assert r.returncode == 255 and "load failure" in r.stdout          # t_exit_code = -1, :479
    bad = tmp_path / "bad.png"
    bad.write_bytes(b"not an image")
    assert run(cli, "--noverbose", bad).returncode == 255
    assert run(cli, "--noverbose", bad).stdout == ""                    # --noverbose silences progress (:372-375)


def test_scale_too_small(cli, tmp_path):
    p = tmp_path / "a.ppm"
    Image.fromarray(np.zeros((3, 3, 3), np.uint8)).save(p)
    r = run(cli, "--scale=0.2", p)                                      # (int)(3*0.2) == 0, :485-495
    assert r.returncode == 255 and "ratio too small" in r.stdout
    r = run(cli, "--scale=-3", "--copy", p, tmp_path / "b.ppm")         # non-positive ratio ignored (:365)
    assert r.returncode == 0


@pytest.mark.parametrize("mode", ["RGB", "L", "RGBA", "P", "LA"])
def test_png_decoder_matches_pil(cli, tmp_path, mode):
    rng = np.random.default_rng(5)
    base = (rng.integers(0, 256, (37, 53, 3)) // 16 * 16).astype(np.uint8)
    base[5:20, 7:30] = [200, 30, 99]                                    # flat areas: exercises all PNG filters
    img = Image.fromarray(base).convert(mode) if mode != "P" else Image.fromarray(base).quantize(64)
    src = tmp_path / f"in_{mode}.png"
    img.save(src)
    want = np.asarray(Image.open(src).convert("RGB"))                   # cv::imread(IMREAD_COLOR): alpha dropped
    for ext in (".ppm", ".png"):
        dst = tmp_path / f"out_{mode}{ext}"
        assert run(cli, "--noverbose", "--copy", src, dst).returncode == 0
        assert np.array_equal(np.asarray(Image.open(dst).convert("RGB")), want)


def test_pnm_reader_and_default_output_name(cli, tmp_path):
    arr = np.random.default_rng(1).integers(0, 256, (9, 14, 3), dtype=np.uint8)
    Image.fromarray(arr).save(tmp_path / "pic.ppm")
    Image.fromarray(arr[:, :, 0]).save(tmp_path / "grey.pgm")
    assert run(cli, "--noverbose", "--copy", "pic.ppm", cwd=tmp_path).returncode == 0
    out = tmp_path / "pic_resized.ppm"                                  # "<name>_resized<ext>", :396-416
    assert out.exists() and np.array_equal(np.asarray(Image.open(out)), arr)
    assert run(cli, "--noverbose", "--copy", "grey.pgm", "g.png", cwd=tmp_path).returncode == 0
    assert np.array_equal(np.asarray(Image.open(tmp_path / "g.png"))[:, :, 1], arr[:, :, 0])


# ---- exits in front of srcnn_create: no GPU needed

ARGUMENT_ERROR_BOGUS = "- argument error : --padding=bogus : expected zero or replicate\n"
MODEL_LOAD_FAILURE = "- model load failure (use --weights=FILE or $SRCNN_WEIGHTS)\n"


@pytest.fixture
def small_ppm(tmp_path):
    Image.fromarray(np.full((6, 8, 3), 90, np.uint8)).save(tmp_path / "a.ppm")
    return tmp_path / "a.ppm"


def test_padding_argument_errors(cli, small_ppm):
    r = run(cli, "--padding=bogus", small_ppm)
    assert r.returncode == 255 and "argument error" in r.stdout and "--padding=bogus" in r.stdout
    r = run(cli, "--padding=zero", "--refbytes", small_ppm)
    assert r.returncode == 255 and "argument error" in r.stdout
    assert "--padding=zero" in r.stdout and "--refbytes" in r.stdout        # names both options
    assert not small_ppm.with_name("a_resized.ppm").exists()


@pytest.mark.parametrize("env_has_a_model", [False, True])
def test_weights_option_is_the_model_or_an_error(cli, small_ppm, tmp_path, env_has_a_model):
    """A file named by --weights= is the model or the run fails: neither a wrong size nor a path that cannot be opened
    falls through to $SRCNN_WEIGHTS or to the shipped 9-1-5 blob (a typo would give a plausible picture from another model)."""
    import srcnn_cpp_amd as S
    env = {"SRCNN_WEIGHTS": S._WEIGHTS_PATH} if env_has_a_model else None
    wrong = tmp_path / "wrong.f32"
    np.zeros(8130, np.float32).tofile(wrong)
    for named in (wrong, tmp_path / "no_such_model.f32"):
        r = run(cli, f"--weights={named}", small_ppm, env=env)
        assert r.returncode == 255 and "model load failure" in r.stdout, r.stdout + r.stderr
        assert not small_ppm.with_name("a_resized.ppm").exists()


def test_noverbose_silences_the_guarded_messages_only(cli, small_ppm, tmp_path):
    """--noverbose empties stdout on the paths that print under `verbose` (source load failure, ratio too small); the argument
    error and the model load failure print whatever the verbosity."""
    r = run(cli, "--noverbose", tmp_path / "missing.png")
    assert r.returncode == 255 and r.stdout == ""
    Image.fromarray(np.zeros((3, 3, 3), np.uint8)).save(tmp_path / "tiny.ppm")
    r = run(cli, "--noverbose", "--scale=0.2", tmp_path / "tiny.ppm")
    assert r.returncode == 255 and r.stdout == ""
    r = run(cli, "--noverbose", "--padding=bogus", small_ppm)
    assert r.returncode == 255 and r.stdout == ARGUMENT_ERROR_BOGUS
    assert run(cli, "--padding=bogus", small_ppm).stdout == ARGUMENT_ERROR_BOGUS      # ... and nothing else with verbose on
    r = run(cli, "--noverbose", f"--weights={tmp_path / 'no_such_model.f32'}", small_ppm)
    assert r.returncode == 255 and r.stdout == MODEL_LOAD_FAILURE
    r = run(cli, f"--weights={tmp_path / 'no_such_model.f32'}", small_ppm)
    assert r.returncode == 255 and r.stdout.endswith(MODEL_LOAD_FAILURE) and "- Image load : " in r.stdout


# ---- the whole tool on the GPU: one picture per process

GOLD = Path(__file__).resolve().parent / "golden"


def synth_bgr(w, h, seed=0):
    from srcnn_cpp_amd.synth import synth_luma
    return np.stack([synth_luma(w, h, frame=seed + k, seed=99 + k) for k in range(3)], axis=2)


def write_bgr(path, bgr):
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path)


def read_bgr(path):
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


@pytest.fixture(scope="module")
def butterfly():
    z = np.load(GOLD / "butterfly_bgr.npz")
    assert z["ref_bgr"].size == 995328
    return z["src_bgr"], z["ref_bgr"]


@pytest.mark.gpu
def test_cli_reference_example_refbytes(cli, tmp_path, butterfly):
    """The reference's documented example, `--scale=1.5 butterfly.png`, through the binary with --refbytes: every byte of
    the reference's published picture, to a .png (the default output name) and to a .ppm."""
    src, ref = butterfly
    write_bgr(tmp_path / "butterfly.png", src)
    r = run(cli, "--scale=1.5", "--refbytes", "butterfly.png", cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    got = read_bgr(tmp_path / "butterfly_resized.png")
    assert got.shape == ref.shape
    n = int((got != ref).sum())
    print(f"butterfly --refbytes: {n} differing bytes of {ref.size}")
    assert n == 0, f"{n} differing bytes of {ref.size}"
    r = run(cli, "--scale=1.5", "--refbytes", "--noverbose", "butterfly.png", "out.ppm", cwd=tmp_path)
    assert r.returncode == 0 and r.stdout == "", r.stdout + r.stderr
    assert (tmp_path / "out.ppm").read_bytes()[:2] == b"P6"
    assert np.array_equal(read_bgr(tmp_path / "out.ppm"), ref)


@pytest.mark.gpu
def test_cli_reference_example_default_mode(cli, tmp_path, butterfly, weights_blob):
    """The same command as most people would type it: the float32 MFMA mode, bitwise the FMA-order model, and within
    test_butterfly_example_on_gpu's bounds of the reference's picture."""
    from cli_reference import expected_bgr_915
    src, ref = butterfly
    write_bgr(tmp_path / "butterfly.png", src)
    r = run(cli, "--scale=1.5", "butterfly.png", cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "- Scale multiply ratio : 1.50" in r.stdout and "- Performace : " in r.stdout
    got = read_bgr(tmp_path / "butterfly_resized.png")
    assert got.shape == ref.shape and np.array_equal(got, expected_bgr_915(src, 1.5, weights_blob, "default"))
    d = np.abs(got.astype(int) - ref.astype(int))
    assert d.max() <= 2
    assert (d.max(axis=2) == 0).mean() >= 0.9995


PICTURE = (96, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["refbytes", "default"])
@pytest.mark.parametrize("scale", [2.0, 3.0, 1.0, 0.75, 0.5, 0.3])
def test_cli_scales_with_the_shipped_model(cli, tmp_path, weights_blob, scale, mode):
    """Up, 1:1 and down (below 1 the pipeline takes the direct resize kernel and the output is smaller than the input):
    --refbytes == the oracle, the default == the FMA-order model, both bitwise, at oracle.scaled_size."""
    import oracle
    from cli_reference import expected_bgr_915
    bgr = synth_bgr(*PICTURE)
    write_bgr(tmp_path / "in.png", bgr)
    r = run(cli, f"--scale={scale}", *(["--refbytes"] if mode == "refbytes" else []), "in.png", cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    got = read_bgr(tmp_path / "in_resized.png")
    ow, oh = oracle.scaled_size(*PICTURE, scale)
    assert got.shape == (oh, ow, 3)
    assert np.array_equal(got, expected_bgr_915(bgr, scale, weights_blob, mode))


# (kind, f2, padding, how the blob reaches the tool).  "both": --weights= names the case's model and $SRCNN_WEIGHTS another
# one (a colour blob, whose picture would fail every check below): --weights= must win.
WEIGHT_CASES = [("luma", 3, "replicate", "option"), ("luma", 5, "replicate", "env"), ("luma", 3, "zero", "both"),
                ("luma", 5, "zero", "option"), ("luma", 1, "zero", "option"),
                ("colour", 1, "replicate", "option"), ("colour", 1, "zero", "option"),
                ("colour", 5, "replicate", "option"), ("colour", 5, "zero", "option")]
BLOB_FLOATS = {("luma", 1): 8129, ("luma", 3): 24513, ("luma", 5): 57281, ("colour", 1): 20099, ("colour", 3): 36483, ("colour", 5): 69251}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,f2,padding,how", WEIGHT_CASES, ids=["-".join(map(str, c)) for c in WEIGHT_CASES])
def test_cli_weight_files(cli, tmp_path, weights_blob, kind, f2, padding, how):
    """Every blob size the tool slices by hand, in both paddings, against float64 restatements built without the product
    (tests/cli_reference.py).  The models give pictures (>= 64 output levels, <= 3 % of the pixels within the tolerance of a
    truncation boundary), so a table read from a wrong offset cannot pass."""
    import cli_reference as R
    from spatial_reference import assert_u8_consistent
    bgr = synth_bgr(*PICTURE)
    write_bgr(tmp_path / "in.png", bgr)
    if kind == "luma":
        model = R.centre_tap_model(weights_blob, f2, 1)
        blob = R.model_blob(model)
        ref_pre, cr, cb = R.luma_reference(bgr, 2.0, model, padding)
    else:
        model = R.centre_tap_color_model(weights_blob, f2, 1)
        blob = R.color_blob(model)
        ref_pre = R.color_reference(bgr, 2.0, model, padding)
    assert blob.size == BLOB_FLOATS[kind, f2] and blob.dtype == np.float32
    if (kind, f2) == ("luma", 1):
        assert np.array_equal(blob, weights_blob)                 # the shipped file, through --weights=
    share = R.assert_is_a_picture(ref_pre)                         # conditions on the case, from the reference alone
    blob.tofile(tmp_path / "model.f32")
    args, env = ["--scale=2.0", f"--padding={padding}"], {}
    if how in ("option", "both"):
        args.append(f"--weights={tmp_path / 'model.f32'}")
    if how == "env":
        env["SRCNN_WEIGHTS"] = tmp_path / "model.f32"
    if how == "both":
        R.color_blob(R.centre_tap_color_model(weights_blob, 1, 2)).tofile(tmp_path / "other.f32")
        env["SRCNN_WEIGHTS"] = tmp_path / "other.f32"
    r = run(cli, *args, "in.png", cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = read_bgr(tmp_path / "in_resized.png")
    print(f"{kind} 9-{f2}-5 {padding}: ambiguous share {share:.4f}")
    if kind == "luma":
        assert R.assert_bgr_of_luma(got, ref_pre, cr, cb) == share
    else:
        assert got.shape == ref_pre.shape, f"(ambiguous share {share:.4f})"
        assert_u8_consistent(got, ref_pre, R.ambiguous(ref_pre)[1])


@pytest.mark.gpu
def test_cli_reports_what_the_library_refuses(cli, tmp_path, weights_blob):
    """--refbytes with a 9-3-5 model: SRCNN_MODE_REFBYTES has no arithmetic for it, the library says so, and the tool passes
    that on -- exit code -10, the library's message, no output file."""
    import cli_reference as R
    write_bgr(tmp_path / "in.png", synth_bgr(*PICTURE))
    R.model_blob(R.centre_tap_model(weights_blob, 3, 1)).tofile(tmp_path / "model.f32")
    r = run(cli, "--refbytes", f"--weights={tmp_path / 'model.f32'}", "in.png", cwd=tmp_path)
    assert r.returncode == 246, r.stdout + r.stderr
    assert "Failure.\n- " in r.stdout
    msg = r.stdout.split("Failure.\n- ", 1)[1]
    assert "a 9-3-5 model runs in SRCNN_MODE_MFMA only" in msg and "mode 3" in msg
    assert not (tmp_path / "in_resized.png").exists()


@pytest.mark.gpu
def test_cli_end_to_end_on_gpu(cli, tmp_path, gpu_ctx):
    from srcnn_cpp_amd.synth import synth_luma
    bgr = np.stack([synth_luma(90, 60, frame=k, seed=7 + k) for k in range(3)], axis=2)
    Image.fromarray(bgr[:, :, ::-1]).save(tmp_path / "in.png")
    r = run(cli, "--scale=1.5", "in.png", cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "- Scale multiply ratio : 1.50" in r.stdout and "- Performace : " in r.stdout and "ms took." in r.stdout
    got = np.asarray(Image.open(tmp_path / "in_resized.png"))[:, :, ::-1]
    assert np.array_equal(got, gpu_ctx.process_bgr(bgr, 1.5))
