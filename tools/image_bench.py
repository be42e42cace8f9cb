"""Time the image calls (CompiledModule.upscale_rgb_image, forward_image: tensors in the format they are stored in) on one GPU
against the existing float32 calls and against the torch conversions a user wraps around those.

    python tools/image_bench.py [--rounds 20] [--warmup 3] [--json profiles/models/image_bench.json]
                                [--rows upscale_rgb forward] [--lib srcnn_cpp_amd/libsrcnn_amd_<variant>.so]

One process, device-resident tensors, one torch stream, HIP events around single calls; the four calls of a row are interleaved
round by round so that clock and neighbour noise hit all of them alike; the figure is the median over the rounds (minimum and
spread = (max - min) / median beside it).  Rows: luma 9-1-5 and 9-5-5 zero-padded models in both modes on a decoded 1920 x 1080
H x W x 3 uint8 picture -> 3840 x 2160 H x W x 3 uint8 (upscale_rgb), and a colour 9-5-5 model on a 3840 x 2160 channels_last
float16 tensor (forward).  Per row:
  1  `f32`          the existing call on planar float32 (upscale_rgb / __call__);
  2  `image_f32`    the new call on the same planar float32 tensor (it must run the same kernels);
  3  `script`       the torch conversions around the existing call for the stored format: conversions in, the call of 1,
                    conversions out;
  4  `image`        the new call on the stored format.
Run the same command twice and compare: 2 / 1 has to sit inside the spread two runs of 1 show, 4 / 3 at or below 1.
No GPU: the tool fails; there is no CPU timing."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402

import srcnn_cpp_amd as S  # noqa: E402
from srcnn_cpp_amd.torch_api import compile_module  # noqa: E402
from resize_f32_bench import stats, timed  # noqa: E402


class SRCNN(torch.nn.Module):
    def __init__(self, f2, channels=1):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(channels, 64, 9, padding=4)
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=f2 // 2)
        self.conv3 = torch.nn.Conv2d(32, channels, 5, padding=2)

    def forward(self, x):
        return self.conv3(torch.relu(self.conv2(torch.relu(self.conv1(x)))))


def rgb_calls(fast, sw, sh, dw, dh):
    """A decoded H x W x 3 uint8 picture in, the same at the target size out."""
    hwc = torch.from_numpy(np.random.default_rng(sw).integers(0, 256, (sh, sw, 3)).astype(np.uint8)).cuda()
    planar = hwc.permute(2, 0, 1).contiguous().float().mul(1.0 / 255.0)
    size, clamp = (dh, dw), (0.0, 1.0)

    def script():
        x = hwc.permute(2, 0, 1).contiguous().float().mul(1.0 / 255.0)
        y = fast.upscale_rgb(x, size=size, clamp=clamp)
        return y.mul(255.0).clamp(0.0, 255.0).round().byte().permute(1, 2, 0).contiguous()
    calls = {"f32": lambda: fast.upscale_rgb(planar, size=size, clamp=clamp),
             "image_f32": lambda: fast.upscale_rgb_image(planar, size=size, clamp=clamp),
             "script": script,
             "image": lambda: fast.upscale_rgb_image(hwc.permute(2, 0, 1), size=size, clamp=clamp)}
    same = bool(torch.equal(calls["image"]().permute(1, 2, 0), script())) and bool(torch.equal(calls["f32"](), calls["image_f32"]()))
    return calls, same


def forward_calls(fast, w, h):
    """A channels_last float16 tensor in, the same out."""
    x16 = torch.from_numpy(np.random.default_rng(w).random((1, 3, h, w), dtype=np.float32)).cuda().half().to(memory_format=torch.channels_last)
    planar = x16.float().contiguous()

    def script():
        return fast(x16.float().contiguous()).half().contiguous(memory_format=torch.channels_last)
    calls = {"f32": lambda: fast(planar), "image_f32": lambda: fast.forward_image(planar), "script": script,
             "image": lambda: fast.forward_image(x16)}
    same = bool(torch.equal(calls["image"](), script())) and bool(torch.equal(calls["f32"](), calls["image_f32"]()))
    return calls, same


def bench(fast, calls, rounds, warmup):
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
    rec = {name: stats(v) for name, v in ms.items()}
    rec["image_f32_over_f32"] = rec["image_f32"]["ms_median"] / rec["f32"]["ms_median"]
    rec["image_over_script"] = rec["image"]["ms_median"] / rec["script"]["ms_median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (srcnn_cpp_amd/build.py, SRCNN_BUILD_VARIANT) for an A/B run")
    ap.add_argument("--rows", nargs="+", default=["upscale_rgb", "forward"], choices=["upscale_rgb", "forward"])
    args = ap.parse_args()
    if args.lib:
        S.use_library(args.lib)
    rows = [r for r in (("upscale_rgb", 1, 1), ("upscale_rgb", 1, 5), ("forward", 3, 5)) if r[0] in args.rows]
    records = []
    for what, channels, f2 in rows:
        torch.manual_seed(f2)
        net = SRCNN(f2, channels).eval()
        for mode, mode_name in ((S.MODE_MFMA, "SRCNN_MODE_MFMA"), (S.MODE_BANDED16, "SRCNN_MODE_BANDED16")):
            fast = compile_module(net, mode=mode, input_range=2.0)          # raises without a gfx950 GPU
            try:
                if what == "upscale_rgb":
                    calls, same = rgb_calls(fast, 1920, 1080, 3840, 2160)
                    label = "H x W x 3 uint8 1920x1080 -> 3840x2160"
                else:
                    calls, same = forward_calls(fast, 3840, 2160)
                    label = "channels_last float16 3840x2160"
                rec = dict(call=what, model=f"{'colour' if channels == 3 else 'luma'} 9-{f2}-5, zero padding", mode=mode_name,
                           stored=label, image_equals_script_bitwise=same, **bench(fast, calls, args.rounds, args.warmup))
                records.append(rec)
                print(f"{rec['model']} {mode_name} {label}: " +
                      ", ".join(f"{k} {rec[k]['ms_median']:.4f} ms ({rec[k]['spread']:.1%})" for k in calls) +
                      f"; image_f32 / f32 {rec['image_f32_over_f32']:.3f}, image / script {rec['image_over_script']:.3f}, "
                      f"bitwise equal to the script: {same}", flush=True)
            finally:
                fast.close()
    result = {"tool": "tools/image_bench.py", "library": args.lib or "the product library", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
              "results": records}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"image_over_script": [r["image_over_script"] for r in records],
                      "image_f32_over_f32": [r["image_f32_over_f32"] for r in records]}))


if __name__ == "__main__":
    main()
