"""Time CompiledModule.upscale_rgb (srcnn_process_rgb_f32_dev: an RGB tensor through a 1-channel model) on one GPU, against the
part of it that existed before and against the torch script it replaces.

    python tools/rgb_f32_bench.py [--shapes 960x540:1920x1080 1920x1080:3840x2160] [--f2 1 5] [--rounds 9] [--inner 6]
                                  [--warmup 3] [--json profiles/models/rgb_f32_bench.json]

Per shape, zero-padded 9-f2-5 model and mode (SRCNN_MODE_MFMA, SRCNN_MODE_BANDED16), four calls are timed in one process on one
torch stream, interleaved round by round so that clock and neighbour noise hit all of them alike (the method of
tools/resize_f32_bench.py: `inner` back-to-back calls between two device events, the figure per round is that time / inner;
median, minimum and spread = (max - min) / median over the rounds):
  a  `rgb`      fast.upscale_rgb(x, size, clamp=(0, 1)) on the (1, 3, h, w) tensor;
  b  `luma`     fast.upscale(y, size) on one plane of the same size: resize + model, the part that already existed;
  c  `script`   the torch script around fast(...): F.interpolate of the three planes, RGB -> Y'CbCr, slice Y, the module, cat,
                Y'CbCr -> RGB, clamp;
  r  `resize3`  the library's float resize of the three planes alone, for its GB/s at the same shape in the same run.
a - b is what the two new kernels cost; its GB/s is over their ALGORITHMIC bytes: front reads 3 source planes and writes 1
output plane, back reads 3 source and 2 output planes and writes 3: 4 B x (6 source + 6 output planes).  The tool also reports
the largest |a - c| at the timed size.  No GPU: the tool fails; there is no CPU timing."""
import argparse
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

# BT.601 full range and its exact inverse, as a script would carry them
M = np.array([[0.299, 0.587, 0.114], [-0.299 * 0.5 / 0.886, -0.587 * 0.5 / 0.886, 0.5], [0.5, -0.587 * 0.5 / 0.701, -0.114 * 0.5 / 0.701]])
MINV = np.linalg.inv(M).tolist()
M = M.tolist()


class SRCNN(torch.nn.Module):
    def __init__(self, f2):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(1, 64, 9, padding=4)
        self.conv2 = torch.nn.Conv2d(64, 32, f2, padding=f2 // 2)
        self.conv3 = torch.nn.Conv2d(32, 1, 5, padding=2)

    def forward(self, x):
        return self.conv3(torch.relu(self.conv2(torch.relu(self.conv1(x)))))


def script(fast, x, size):
    """What a torch user writes around a luma model."""
    up = F.interpolate(x, size=size, mode="bicubic", align_corners=False)
    r, g, b = up[:, 0:1], up[:, 1:2], up[:, 2:3]
    y = M[0][0] * r + M[0][1] * g + M[0][2] * b
    cb = M[1][0] * r + M[1][1] * g + M[1][2] * b + 0.5
    cr = M[2][0] * r + M[2][1] * g + M[2][2] * b + 0.5
    ycc = torch.cat([fast(y), cb - 0.5, cr - 0.5], dim=1)
    y2, cb2, cr2 = ycc[:, 0:1], ycc[:, 1:2], ycc[:, 2:3]
    out = torch.cat([MINV[c][0] * y2 + MINV[c][1] * cb2 + MINV[c][2] * cr2 for c in range(3)], dim=1)
    return out.clamp(0.0, 1.0)


def bench_shape(fast, sw, sh, dw, dh, rounds, inner, warmup):
    rng = np.random.default_rng(sw)
    x = torch.from_numpy(rng.random((1, 3, sh, sw), dtype=np.float32)).cuda()
    y = x[:, :1].contiguous()
    up3 = torch.empty((1, 3, dh, dw), dtype=torch.float32, device="cuda")
    sp, dp = sw * sh, dw * dh
    calls = {
        "rgb": lambda: fast.upscale_rgb(x, size=(dh, dw), clamp=(0.0, 1.0)),
        "luma": lambda: fast.upscale(y, size=(dh, dw)),
        "script": lambda: script(fast, x, (dh, dw)),
        "resize3": lambda: fast.ctx.resize_cubic_f32_dev(x.data_ptr(), sw, sp, 0, sw, sh, up3.data_ptr(), dw, dp, 0, dw, dh, 3, 1),
    }
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ms = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        fast.ctx.set_stream(stream.cuda_stream)          # (resize3 goes to the context directly)
        for run in calls.values():
            for _ in range(warmup):
                run()
        stream.synchronize()
        diff = float((calls["rgb"]() - calls["script"]()).abs().max())
        for _ in range(rounds):
            for name, run in calls.items():
                ms[name].append(timed(stream, run, inner))
    rec = {"src": [sw, sh], "dst": [dw, dh], "max_abs_rgb_minus_script": diff}
    for name in calls:
        rec[name] = stats(ms[name])
    extra = np.array(ms["rgb"]) - np.array(ms["luma"])
    nbytes = 4.0 * 6 * (sp + dp)
    rec["rgb_minus_luma"] = {"us_median": float(np.median(extra)) * 1e3, "us_min": float(extra.min()) * 1e3, "us_max": float(extra.max()) * 1e3,
                             "algorithmic_bytes": nbytes, "algorithmic_GBps": nbytes / (float(np.median(extra)) * 1e-3) / 1e9}
    rec["resize3"]["algorithmic_GBps"] = 4.0 * 3 * (sp + dp) / (rec["resize3"]["ms_median"] * 1e-3) / 1e9
    rec["rgb_over_script"] = rec["rgb"]["ms_median"] / rec["script"]["ms_median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["960x540:1920x1080", "1920x1080:3840x2160"])
    ap.add_argument("--f2", type=int, nargs="+", default=[1, 5], choices=[1, 3, 5])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    shapes = []
    for s in args.shapes:
        a, b = s.split(":")
        shapes.append(tuple(int(v) for v in a.split("x")) + tuple(int(v) for v in b.split("x")))
    records = []
    for f2 in args.f2:
        torch.manual_seed(f2)
        net = SRCNN(f2).eval()
        for mode, mode_name in ((S.MODE_MFMA, "SRCNN_MODE_MFMA"), (S.MODE_BANDED16, "SRCNN_MODE_BANDED16")):
            fast = compile_module(net, mode=mode, input_range=2.0)          # raises without a gfx950 GPU: nothing is timed on a CPU
            try:
                for sw, sh, dw, dh in shapes:
                    rec = dict(model=f"9-{f2}-5, zero padding", mode=mode_name, **bench_shape(fast, sw, sh, dw, dh, args.rounds,
                                                                                            args.inner, args.warmup))
                    records.append(rec)
                    d = rec["rgb_minus_luma"]
                    print(f"9-{f2}-5 {mode_name} {sw}x{sh} -> {dw}x{dh}: rgb {rec['rgb']['ms_median']:.4f} ms (spread "
                          f"{rec['rgb']['spread']:.1%}), luma {rec['luma']['ms_median']:.4f} ms, rgb - luma {d['us_median']:.1f} us "
                          f"[{d['us_min']:.1f}, {d['us_max']:.1f}] = {d['algorithmic_GBps']:.0f} GB/s; resize3 "
                          f"{rec['resize3']['ms_median']:.4f} ms = {rec['resize3']['algorithmic_GBps']:.0f} GB/s; script "
                          f"{rec['script']['ms_median']:.4f} ms (spread {rec['script']['spread']:.1%}), rgb / script "
                          f"{rec['rgb_over_script']:.3f}; max|rgb - script| {rec['max_abs_rgb_minus_script']:.3g}", flush=True)
            finally:
                fast.close()
    result = {"tool": "tools/rgb_f32_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner,
              "warmup": args.warmup, "luma": "BT.601 full range, clamp (0, 1), data uniform [0, 1)",
              "bytes": "algorithmic, rgb - luma: 4 B x (6 source planes + 6 output planes); resize3: 4 B x 3 x (source + output)",
              "results": records}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"rgb_over_script": [r["rgb_over_script"] for r in records]}))


if __name__ == "__main__":
    main()
