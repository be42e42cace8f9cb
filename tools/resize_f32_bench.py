"""Time the float32 cubic resize (srcnn_resize_cubic_f32_dev) and resize + model (srcnn_process_f32_dev) on one GPU, against
what a user has without them: torch.nn.functional.interpolate(mode="bicubic", align_corners=False) on the same CUDA tensor.

    python tools/resize_f32_bench.py [--shapes 960x540:1920x1080 1920x1080:3840x2160] [--channels 1 3] [--rounds 9]
                                     [--inner 20] [--warmup 3] [--json profiles/models/resize_f32_bench.json]

Per shape and channel count, four calls are timed in one process on one torch stream, interleaved round by round so that
clock and neighbour noise hit all of them alike: `resize` (the library), `torch` (F.interpolate), `process` (resize + model)
and `forward` (srcnn_forward_f32_dev on the already resized planes: process should cost resize + forward and nothing else).
One measurement is `inner` back-to-back calls between two device events (a single resize is tens of microseconds: one call
between two events would time the events); the figure per round is that time / inner.  Reported per call: the median, the
minimum and the spread (max - min over the rounds, as a fraction of the median).  GB/s is ALGORITHMIC bytes over the median:
4 B written per output element and 4 B read per source element.  The tool also compares the library's output with torch's
at the timed size (torch computes its coordinates in float32: a difference of a few 1e-5 x max|x| is its drift).
No GPU: the tool fails; there is no CPU timing."""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402

import srcnn_cpp_amd as S  # noqa: E402
from model_bench import color_model, model  # noqa: E402


def timed(stream, run, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(inner):
        run()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(ms):
    med = float(np.median(ms))
    return {"ms_median": med, "ms_min": float(np.min(ms)), "spread": float((np.max(ms) - np.min(ms)) / med), "rounds": len(ms)}


def bench_shape(ctx, sw, sh, dw, dh, channels, rounds, inner, warmup):
    rng = np.random.default_rng(sw + channels)
    x = torch.from_numpy(rng.random((1, channels, sh, sw), dtype=np.float32) * np.float32(255.0)).cuda()
    up = torch.empty((1, channels, dh, dw), dtype=torch.float32, device="cuda")
    out = torch.empty_like(up)
    ctx.set_model(*(color_model(1) if channels == 3 else model(1)))
    sp, dp = sw * sh, dw * dh
    calls = {
        "resize": lambda: ctx.resize_cubic_f32_dev(x.data_ptr(), sw, sp, 0, sw, sh, up.data_ptr(), dw, dp, 0, dw, dh, channels, 1),
        "torch": lambda: F.interpolate(x, size=(dh, dw), mode="bicubic", align_corners=False),
        "process": lambda: ctx.process_f32_dev(x.data_ptr(), sw, sp, 0, sw, sh, out.data_ptr(), dw, dp, 0, dw, dh, 1),
        "forward": lambda: ctx.forward_f32_dev(up.data_ptr(), dw, dp, 0, out.data_ptr(), dw, dp, 0, dw, dh, 1),
    }
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ms = {k: [] for k in calls}
    try:
        with torch.cuda.stream(stream):
            for run in calls.values():
                for _ in range(warmup):
                    run()
            stream.synchronize()
            diff = float((up - calls["torch"]()).abs().max())
            for _ in range(rounds):
                for name, run in calls.items():
                    ms[name].append(timed(stream, run, inner if name in ("resize", "torch") else max(1, inner // 4)))
    finally:
        ctx.set_stream(0)
    rec = {"src": [sw, sh], "dst": [dw, dh], "channels": channels, "max_abs_diff_vs_torch": diff, "max_abs_x": 255.0}
    nbytes = 4.0 * channels * (sp + dp)
    for name in calls:
        rec[name] = stats(ms[name])
    for name in ("resize", "torch"):
        rec[name]["algorithmic_GBps"] = nbytes / (rec[name]["ms_median"] * 1e-3) / 1e9
    rec["resize_over_torch"] = rec["resize"]["ms_median"] / rec["torch"]["ms_median"]
    rec["process_over_resize_plus_forward"] = rec["process"]["ms_median"] / (rec["resize"]["ms_median"] + rec["forward"]["ms_median"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["960x540:1920x1080", "1920x1080:3840x2160"])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 3], choices=[1, 3])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    shapes = []
    for s in args.shapes:
        a, b = s.split(":")
        shapes.append(tuple(int(v) for v in a.split("x")) + tuple(int(v) for v in b.split("x")))
    records = []
    with S.Context(0) as ctx:                   # raises without a gfx950 GPU: nothing is timed on a CPU
        ctx.set_mode(S.MODE_MFMA)
        for sw, sh, dw, dh in shapes:
            for channels in args.channels:
                rec = bench_shape(ctx, sw, sh, dw, dh, channels, args.rounds, args.inner, args.warmup)
                records.append(rec)
                print(f"{sw}x{sh} -> {dw}x{dh} x{channels}: resize {rec['resize']['ms_median']:.4f} ms "
                      f"({rec['resize']['algorithmic_GBps']:.0f} GB/s, spread {rec['resize']['spread']:.1%}), torch "
                      f"{rec['torch']['ms_median']:.4f} ms (spread {rec['torch']['spread']:.1%}), ratio {rec['resize_over_torch']:.3f}; "
                      f"process {rec['process']['ms_median']:.4f} ms = {rec['process_over_resize_plus_forward']:.3f} x (resize + forward "
                      f"{rec['forward']['ms_median']:.4f}); max|resize - torch| {rec['max_abs_diff_vs_torch']:.3g}", flush=True)
    result = {"tool": "tools/resize_f32_bench.py", "device": torch.cuda.get_device_name(0), "mode": "SRCNN_MODE_MFMA, 9-1-5, replicate padding",
              "rounds": args.rounds, "inner": args.inner, "warmup": args.warmup,
              "bytes": "algorithmic: 4 B per output element written + 4 B per source element read", "results": records}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"resize_over_torch": [r["resize_over_torch"] for r in records]}))


if __name__ == "__main__":
    main()
