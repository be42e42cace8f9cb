"""Time the full-reference metrics (CompiledModule.metrics: squared error and Gaussian-window SSIM in float64) on one GPU against
the torch script users run for the same numbers, on the same tensors in the same process.

    python tools/metrics_bench.py [--rounds 20] [--warmup 3] [--border 2] [--json profiles/models/metrics_bench.json]

One process, device-resident tensors, one torch stream, HIP events around single calls; the calls of a row are interleaved round
by round so that clock and neighbour noise hit both alike; the figure is the median over the rounds (minimum and spread =
(max - min) / median beside it).  Rows: a pair of 3840 x 2160 pictures as one float32 plane, as three float32 planes, and as
H x W x 3 uint8 measured on the BT.601 luma; each for the squared error alone and for squared error + SSIM.  Per row:
  `lib`      the library's call: both pictures read where they lie, float64 after the load, four doubles per result;
  `torch`    the script in FLOAT32 -- the form users run and the one favourable to torch: conversion and luma for uint8, the border
             sliced off, ((a - b) ** 2).sum(), five conv2d with the 11 x 11 Gaussian window, the SSIM map and its sum.
Before a row is timed the library's result is checked against the same script in float64 (separable window sums on .double()
tensors): relative error of the squared error <= (n + 4) 2^-53, mean SSIM within 1e-9.  Beside the times: the bytes of both pictures read once.  Run the same command twice and compare; per-kernel
times come from a run of its own under rocprofv3 --kernel-trace --stats.
--msssim times MS-SSIM instead (CompiledModule.msssim_sums, five scales; profiles/models/msssim_bench.json is its --json): the
same three pictures, one row each, against (a) `torch`, the float32 script of the same metric (five
rounds of the five conv2d, avg_pool2d(2) between them), and (b) `ssim`, the library's own metrics(ssim=True) of the same pair.
Before a row is timed the sums are checked against the metric in float64 (the same separable sums, the 2 x 2 mean with an odd
last row or column paired with itself): per-scale mean cs and mean SSIM within 1e-9.
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
from srcnn_cpp_amd.torch_api import compile_module  # noqa: E402
from resize_f32_bench import stats, timed  # noqa: E402

SIZE = (2160, 3840)
SSIM_TOL = 1e-9


class SRCNN(torch.nn.Module):      # the metrics need no model; compile_module needs a module to own the context
    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(1, 64, 9, padding=4)
        self.conv2 = torch.nn.Conv2d(64, 32, 1)
        self.conv3 = torch.nn.Conv2d(32, 1, 5, padding=2)


def window(dtype):
    g = torch.tensor([np.exp(-((i - 5) ** 2) / 4.5) for i in range(11)], dtype=torch.float64)
    return (g / g.sum()).to(dtype).cuda()


def planes(x, luma, border, dtype):
    """(N, C, H, W) stored tensor -> the measured planes (N, P, h', w') in dtype, as a script does it"""
    x = x.to(dtype) * (1.0 / 255.0) if x.dtype == torch.uint8 else x.to(dtype)
    if luma is not None:
        w = torch.tensor(luma, dtype=torch.float32).to(dtype)
        x = (((w[0] * x[:, 0] + w[1] * x[:, 1]) + w[2] * x[:, 2]) + w[3]).unsqueeze(1)
    return x[..., border:x.shape[-2] - border, border:x.shape[-1] - border] if border else x


def script32(a, b, luma, border, ssim):
    """The yardstick: float32 throughout, conv2d with the 2-D window"""
    a, b = planes(a, luma, border, torch.float32), planes(b, luma, border, torch.float32)
    sse = ((a - b) ** 2).sum(dim=(-2, -1))
    if not ssim:
        return sse
    c = a.shape[1]
    g = window(torch.float32)
    win = torch.outer(g, g)[None, None].repeat(c, 1, 1, 1)
    blur = lambda t: F.conv2d(t, win, groups=c)
    ma, mb, eaa, ebb, eab = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * ma * mb + c1) * (2 * (eab - ma * mb) + c2)) / ((ma * ma + mb * mb + c1) * ((eaa - ma * ma) + (ebb - mb * mb) + c2))
    return sse, m.sum(dim=(-2, -1))


def script64(a, b, luma, border):
    """The check: float64 throughout, the window applied separably by shifted slices"""
    if a.dtype == torch.uint8:      # the library loads a byte as float32(b) * float32(1 / 255)
        a, b = a.float() * (1.0 / 255.0), b.float() * (1.0 / 255.0)
    a, b = planes(a, luma, border, torch.float64), planes(b, luma, border, torch.float64)
    g = window(torch.float64)

    def blur(t):
        n = t.shape[-2] - 10
        v = sum(g[j] * t[..., j:j + n, :] for j in range(11))
        n = t.shape[-1] - 10
        return sum(g[j] * v[..., j:j + n] for j in range(11))
    ma, mb, eaa, ebb, eab = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * ma * mb + c1) * (2 * (eab - ma * mb) + c2)) / ((ma * ma + mb * mb + c1) * ((eaa - ma * ma) + (ebb - mb * mb) + c2))
    return ((a - b) ** 2).sum(dim=(-2, -1)), m.mean(dim=(-2, -1))


N_SCALES = 5


def ms_script32(a, b, luma, border):
    """The yardstick for MS-SSIM: float32 throughout, conv2d with the 2-D window, avg_pool2d between the scales"""
    a, b = planes(a, luma, border, torch.float32), planes(b, luma, border, torch.float32)
    c = a.shape[1]
    g = window(torch.float32)
    win = torch.outer(g, g)[None, None].repeat(c, 1, 1, 1)
    blur = lambda t: F.conv2d(t, win, groups=c)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    out = []
    for s in range(N_SCALES):
        ma, mb, eaa, ebb, eab = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
        cs = (2 * (eab - ma * mb) + c2) / ((eaa - ma * ma) + (ebb - mb * mb) + c2)
        out.append((cs.sum(dim=(-2, -1)), (cs * (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)).sum(dim=(-2, -1))))
        if s + 1 < N_SCALES:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return out


def ms_script64(a, b, luma, border):
    """The check for MS-SSIM: float64 throughout, separable window sums, the library's reduction -> (N, P, S, 2) means"""
    if a.dtype == torch.uint8:      # the library loads a byte as float32(b) * float32(1 / 255)
        a, b = a.float() * (1.0 / 255.0), b.float() * (1.0 / 255.0)
    a, b = planes(a, luma, border, torch.float64), planes(b, luma, border, torch.float64)
    g = window(torch.float64)

    def blur(t):
        n = t.shape[-2] - 10
        v = sum(g[j] * t[..., j:j + n, :] for j in range(11))
        n = t.shape[-1] - 10
        return sum(g[j] * v[..., j:j + n] for j in range(11))

    def reduce2(t):      # an odd last row or column once more, then the 2 x 2 mean
        t = F.pad(t, (0, t.shape[-1] % 2, 0, t.shape[-2] % 2), mode="replicate")
        return ((t[..., 0::2, 0::2] + t[..., 0::2, 1::2]) + (t[..., 1::2, 0::2] + t[..., 1::2, 1::2])) * 0.25
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    out = []
    for s in range(N_SCALES):
        ma, mb, eaa, ebb, eab = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
        cs = (2 * (eab - ma * mb) + c2) / ((eaa - ma * ma) + (ebb - mb * mb) + c2)
        ssim = ((2 * ma * mb + c1) * (2 * (eab - ma * mb) + c2)) / ((ma * ma + mb * mb + c1) * ((eaa - ma * ma) + (ebb - mb * mb) + c2))
        out.append(torch.stack((cs.mean(dim=(-2, -1)), ssim.mean(dim=(-2, -1))), dim=-1))
        del ma, mb, eaa, ebb, eab, cs, ssim
        if s + 1 < N_SCALES:
            a, b = reduce2(a), reduce2(b)
    return torch.stack(out, dim=-2)


def msssim_rows(fast, args):
    records = []
    for stored in ("float32, 1 plane", "float32, 3 planes", "H x W x 3 uint8, BT.601 luma"):
        a, b, luma, nbytes = pictures(stored)
        got = fast.msssim_sums(a, b, border=args.border, luma=luma, n_scales=N_SCALES).cpu().numpy()
        want = ms_script64(a, b, luma, args.border).cpu().numpy()
        torch.cuda.empty_cache()
        err = float(max(np.abs(got[..., 0] / got[..., 2] - want[..., 0]).max(), np.abs(got[..., 1] / got[..., 2] - want[..., 1]).max()))
        if err > SSIM_TOL:
            raise SystemExit(f"{stored}: per-scale means off by {err:.3g}: nothing timed")
        calls = {"lib": lambda: fast.msssim_sums(a, b, border=args.border, luma=luma, n_scales=N_SCALES),
                 "torch": lambda: ms_script32(a, b, luma, args.border),
                 "ssim": lambda: fast.metrics(a, b, border=args.border, luma=luma, ssim=True)}
        rec = dict(stored=stored, size=f"{SIZE[1]}x{SIZE[0]}", border=args.border, metric=f"MS-SSIM, {N_SCALES} scales",
                   scale_means_err_vs_float64=err, bytes_read_once=nbytes, **bench(calls, args.rounds, args.warmup))
        rec["lib_over_torch"] = rec["lib"]["ms_median"] / rec["torch"]["ms_median"]
        rec["lib_over_ssim"] = rec["lib"]["ms_median"] / rec["ssim"]["ms_median"]
        records.append(rec)
        print(f"{stored}, {rec['metric']} ({nbytes / 1e6:.1f} MB): " +
              ", ".join(f"{k} {rec[k]['ms_median']:.4f} ms (min {rec[k]['ms_min']:.4f}, {rec[k]['spread']:.1%})" for k in calls) +
              f"; lib / torch {rec['lib_over_torch']:.3f}, lib / ssim {rec['lib_over_ssim']:.3f}; |scale means - float64| {err:.3g}", flush=True)
        del a, b
        torch.cuda.empty_cache()
    return records


def pictures(stored):
    h, w = SIZE
    rng = np.random.default_rng(len(stored))
    if "uint8" in stored:
        a = rng.integers(0, 256, (1, h, w, 3)).astype(np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
        return (torch.from_numpy(a).cuda().permute(0, 3, 1, 2), torch.from_numpy(b).cuda().permute(0, 3, 1, 2), S.LUMA_BT601, 6 * h * w)
    c = 3 if "3 planes" in stored else 1
    a = rng.random((1, c, h, w), dtype=np.float32)
    b = np.clip(a + 0.02 * rng.standard_normal(a.shape).astype(np.float32), 0.0, 1.0)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), None, 8 * c * h * w


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
    ap.add_argument("--border", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library")
    ap.add_argument("--msssim", action="store_true", help="time MS-SSIM (five scales) instead of the squared error and SSIM")
    args = ap.parse_args()
    if args.lib:
        S.use_library(args.lib)
    fast = compile_module(SRCNN().eval())          # raises without a gfx950 GPU
    records = []
    try:
        if args.msssim:
            records = msssim_rows(fast, args)
        for stored in () if args.msssim else ("float32, 1 plane", "float32, 3 planes", "H x W x 3 uint8, BT.601 luma"):
            a, b, luma, nbytes = pictures(stored)
            got = fast.metrics(a, b, border=args.border, luma=luma).cpu().numpy()
            sse64, ssim64 = (t.cpu().numpy() for t in script64(a, b, luma, args.border))
            n_px = got[..., 1]
            sse_err = float((np.abs(got[..., 0] - sse64) / sse64).max())
            ssim_err = float(np.abs(got[..., 2] / got[..., 3] - ssim64).max())
            if sse_err > (n_px.max() + 4) * 2.0 ** -53 or ssim_err > SSIM_TOL:
                raise SystemExit(f"{stored}: squared error off by {sse_err:.3g} (relative), mean SSIM by {ssim_err:.3g}: nothing timed")
            for ssim in (False, True):
                calls = {"lib": lambda: fast.metrics(a, b, border=args.border, luma=luma, ssim=ssim),
                         "torch": lambda: script32(a, b, luma, args.border, ssim)}
                rec = dict(stored=stored, size=f"{SIZE[1]}x{SIZE[0]}", border=args.border, metric="SSE + SSIM" if ssim else "SSE",
                           sse_rel_err_vs_float64=sse_err, mean_ssim_err_vs_float64=ssim_err, bytes_read_once=nbytes,
                           **bench(calls, args.rounds, args.warmup))
                for k in calls:
                    rec[k]["GB_per_s"] = nbytes / rec[k]["ms_median"] / 1e6
                rec["lib_over_torch"] = rec["lib"]["ms_median"] / rec["torch"]["ms_median"]
                records.append(rec)
                print(f"{stored}, {rec['metric']} ({nbytes / 1e6:.1f} MB): " +
                      ", ".join(f"{k} {rec[k]['ms_median']:.4f} ms ({rec[k]['spread']:.1%}, {rec[k]['GB_per_s']:.0f} GB/s)" for k in calls) +
                      f"; lib / torch {rec['lib_over_torch']:.3f}; SSE rel. err {sse_err:.3g}, |mean SSIM - float64| {ssim_err:.3g}",
                      flush=True)
            del a, b
            torch.cuda.empty_cache()
    finally:
        fast.close()
    result = {"tool": "tools/metrics_bench.py", "library": args.lib or "the product library", "device": torch.cuda.get_device_name(0),
              "rounds": args.rounds, "warmup": args.warmup, "results": records}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    summary = {"lib_over_torch": [r["lib_over_torch"] for r in records]}
    if args.msssim:
        summary["lib_over_ssim"] = [r["lib_over_ssim"] for r in records]
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
