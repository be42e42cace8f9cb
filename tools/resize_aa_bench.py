"""Time the antialiased cubic resize (CompiledModule.resize / resize_image with antialias=True) on one GPU against torch's own
kernel, F.interpolate(mode="bicubic", align_corners=False, antialias=True), on the same tensor in the same process.

    python tools/resize_aa_bench.py [--rounds 20] [--warmup 3] [--json profiles/models/resize_aa_bench.json]
                                    [--lib srcnn_cpp_amd/libsrcnn_amd_tuning.so --general]

One process, device-resident tensors, one torch stream, HIP events around single calls; the calls of a row are interleaved round
by round so that clock and neighbour noise hit all of them alike; the figure is the median over the rounds (minimum and spread =
(max - min) / median beside it).  Rows: a 3840 x 2160 picture -> 1920 x 1080 and -> 2560 x 1440 as one float32 plane, three
float32 planes, and H x W x 3 uint8 in and out.  Per row:
  `aa`       the library's call (the tiled form: both ratios are below 4);
  `torch`    F.interpolate(..., antialias=True) on the same tensor; for uint8 with the torch conversions around it (permute, float,
             scale in; scale, clamp, round, byte, permute out);
  `general`  with --general (the tuning build: the form hook lives there only): the library's call forced to its two-launch form.
Before anything is timed the library's result is checked against F.interpolate on float64 (2e-6 x max|x|; uint8: at most one
byte step from torch's own result, whose float32 arithmetic drifts by up to 4e-6).  Beside the times: the algorithmic bytes
(source read once, destination written once) and the bandwidth they imply at the median.  Run the same command twice and
compare; per-kernel times come from a run of its own under rocprofv3 --kernel-trace --stats.
No GPU: the tool fails; there is no CPU timing."""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402

import srcnn_cpp_amd as S  # noqa: E402
from srcnn_cpp_amd.torch_api import compile_module  # noqa: E402
from resize_f32_bench import stats, timed  # noqa: E402

TOL = 2e-6
SRC = (2160, 3840)
TARGETS = [(1080, 1920), (1440, 2560)]


class SRCNN(torch.nn.Module):      # the resize needs no model; compile_module needs a module to own the context
    def __init__(self, channels):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(channels, 64, 9, padding=4)
        self.conv2 = torch.nn.Conv2d(64, 32, 1)
        self.conv3 = torch.nn.Conv2d(32, channels, 5, padding=2)


def torch_aa(x, size):
    return F.interpolate(x, size=size, mode="bicubic", align_corners=False, antialias=True)


def float_row(fast, channels, size):
    sh, sw = SRC
    x = torch.from_numpy(np.random.default_rng(channels + size[0]).random((1, channels, sh, sw), dtype=np.float32)).cuda()
    calls = {"aa": lambda: fast.resize(x, size, antialias=True), "torch": lambda: torch_aa(x, size)}
    ref = torch_aa(x.double().cpu(), size)
    err = float((calls["aa"]().double().cpu() - ref).abs().max())
    nbytes = 4 * channels * (sh * sw + size[0] * size[1])
    return calls, err, err <= TOL * float(x.max()), nbytes


def u8_row(fast, size):
    sh, sw = SRC
    hwc = torch.from_numpy(np.random.default_rng(size[0]).integers(0, 256, (sh, sw, 3)).astype(np.uint8)).cuda()

    def script():
        x = hwc.permute(2, 0, 1).unsqueeze(0).float().mul(1.0 / 255.0)
        return torch_aa(x, size).mul(255.0).clamp(0.0, 255.0).round().byte()[0].permute(1, 2, 0).contiguous()
    calls = {"aa": lambda: fast.resize_image(hwc.permute(2, 0, 1), size, antialias=True).permute(1, 2, 0), "torch": script}
    x64 = hwc.permute(2, 0, 1).unsqueeze(0).float().mul(1.0 / 255.0).double().cpu()
    loaded = fast.resize_image(hwc.permute(2, 0, 1), size, out_dtype=torch.float32, antialias=True)
    err = float((loaded.double().cpu() - torch_aa(x64, size)[0]).abs().max())
    step = int((calls["aa"]().int() - script().int()).abs().max())
    return calls, err, err <= TOL and step <= 1, 3 * (sh * sw + size[0] * size[1])


def bench(calls, rounds, warmup):
    stream = torch.cuda.Stream()
    ms = {k: [] for k in calls}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for run in calls.values():
            for _ in range(warmup):
                run()
        stream.synchronize()
        for _ in range(rounds):
            for name, run in calls.items():
                ms[name].append(timed(stream, run, 1))
    return {name: stats(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (the tuning build for --general)")
    ap.add_argument("--general", action="store_true", help="also time the two-launch form (needs --lib <the tuning build>)")
    args = ap.parse_args()
    if args.lib:
        S.use_library(args.lib)
    form = None
    if args.general:
        form = S.load_library().srcnn_debug_resample_aa_form          # AttributeError in the product library
        form.argtypes = [ctypes.c_int]
    fast = {c: compile_module(SRCNN(c).eval()) for c in (1, 3)}          # raises without a gfx950 GPU
    records = []
    try:
        for size in TARGETS:
            for stored, channels in (("float32, 1 plane", 1), ("float32, 3 planes", 3), ("H x W x 3 uint8", 3)):
                calls, err, ok, nbytes = u8_row(fast[3], size) if "uint8" in stored else float_row(fast[channels], channels, size)
                if not ok:
                    raise SystemExit(f"{stored} -> {size}: the result is {err:.3g} from torch's float64 result: nothing timed")
                if form is not None:
                    aa = calls["aa"]
                    calls["general"] = lambda aa=aa: (form(0), aa(), form(-1))[1]
                rec = dict(stored=stored, source=f"{SRC[1]}x{SRC[0]}", target=f"{size[1]}x{size[0]}", max_err_vs_float64=err,
                           algorithmic_bytes=nbytes, **bench(calls, args.rounds, args.warmup))
                for k in calls:
                    rec[k]["GB_per_s"] = nbytes / rec[k]["ms_median"] / 1e6
                rec["aa_over_torch"] = rec["aa"]["ms_median"] / rec["torch"]["ms_median"]
                records.append(rec)
                print(f"{stored} {rec['source']} -> {rec['target']} ({nbytes / 1e6:.1f} MB): " +
                      ", ".join(f"{k} {rec[k]['ms_median']:.4f} ms ({rec[k]['spread']:.1%}, {rec[k]['GB_per_s']:.0f} GB/s)" for k in calls) +
                      f"; aa / torch {rec['aa_over_torch']:.3f}; |aa - float64| {err:.3g}", flush=True)
    finally:
        for f in fast.values():
            f.close()
    result = {"tool": "tools/resize_aa_bench.py", "library": args.lib or "the product library", "device": torch.cuda.get_device_name(0),
              "rounds": args.rounds, "warmup": args.warmup, "results": records}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"aa_over_torch": [r["aa_over_torch"] for r in records]}))


if __name__ == "__main__":
    main()
