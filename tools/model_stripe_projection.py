#!/usr/bin/env python3
"""What ONE rank of a row-striped plane does at N = 1 / 2 / 4 / 8 for the 9-3-5 and 9-5-5 models, timed on one GPU -- after
tools/stripe_projection.py, which does the same for the 9-1-5 strip path.

For every model (9-5-5, 9-3-5), mode (SRCNN_MODE_MFMA, SRCNN_MODE_BANDED16), N and rank k of a 7680x4320 plane this runs exactly
that rank's step ALONE on the GPU: srcnn_model_rows_halo_dev on its rows srcnn_stripe_rows(H, N, k), the halo pointers aimed at
the neighbouring rows of the plane where they lie (the same-device / peer-access transport: no copy).  HIP events around each
call on the context's stream; warm-up calls, then the median of --steps calls.  N = 1 is srcnn_model_rows_dev on the whole
plane; the whole-plane call srcnn_forward_y_dev is timed in the same run as the baseline, at 7680x4320 and at 3840x2160, the
size profiles/models/banded16_bench.json holds (tools/model_bench.py's models, replicate padding), so that a whole-plane figure
that moved shows.

A rank recomputes the rows its bands share with the neighbours': 2 + r2 layer-1 rows and 2 layer-2 rows at each side that
has a neighbour.  Beside the measured overhead of the slowest rank, N t_k(N) / t(1), the tool prints the ratio those rows
predict for each layer, (rows + s (2 + r2)) / rows for layer 1 and (rows + 2 s) / rows for layer 2, s = the sides with a
neighbour; the measurement should lie between 1 and the larger of the two (layer 3 recomputes nothing).

usage: python tools/model_stripe_projection.py [--width 7680 --height 4320 --steps 20 --warmup 3] [--json out.json]
"""
import argparse
import json
import sys
from pathlib import Path

import torch  # noqa: F401  -- before the HIP library: one HIP runtime for both

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

import srcnn_cpp_amd as S  # noqa: E402
from srcnn_cpp_amd.synth import synth_luma  # noqa: E402

sys.path.insert(0, str(ROOT / "tools"))
from model_bench import model  # noqa: E402

MODES = {"mfma": S.MODE_MFMA, "banded16": S.MODE_BANDED16}


def timed(stream, ctx, run, steps, warmup):
    """(median, min, max) ms of `steps` calls, one pair of events per call, after `warmup` calls."""
    for _ in range(warmup):
        run()
    ctx.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        run()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns", default="1,2,4,8")
    ap.add_argument("--f2", type=int, nargs="+", default=[5, 3], choices=[3, 5])
    ap.add_argument("--modes", nargs="+", default=["mfma", "banded16"], choices=list(MODES))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: the median of at least 20 calls")
    W, H = args.width, args.height
    ns = [int(x) for x in args.ns.split(",")]
    ctx = S.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    d_plane = torch.from_numpy(synth_luma(W, H)).cuda()
    d_whole = torch.zeros_like(d_plane)
    d_out = torch.zeros_like(d_plane)
    bw, bh = 3840, 2160                          # the size of profiles/models/banded16_bench.json
    d_small = torch.from_numpy(synth_luma(bw, bh)).cuda()
    d_small_out = torch.zeros_like(d_small)
    recorded = {}
    try:
        for e in json.loads((ROOT / "profiles" / "models" / "banded16_bench.json").read_text()):
            if e["channels"] == 1 and e["padding"] == "replicate" and (e["width"], e["height"]) == (bw, bh):
                recorded[e["model"]] = {"mfma": e["ms_per_plane"], "banded16": e["ms_per_plane_banded16"]}
    except OSError:
        pass
    torch.cuda.synchronize()
    results = []
    print(f"# tools/model_stripe_projection.py: {W}x{H} plane, one MI355X, median of {args.steps} calls after {args.warmup} warm-up calls")
    for f2 in args.f2:
        r2 = (f2 - 1) // 2
        ctx.set_model(*model(f2))
        R = ctx.model_halo_rows()
        for mode in args.modes:
            ctx.set_mode(MODES[mode])
            name = f"9-{f2}-5"
            # baselines of the same run: the whole-plane call, here and at the size of the recorded benchmark
            t_small = timed(stream, ctx, lambda: ctx.forward_y_dev(d_small.data_ptr(), bw, 0, d_small_out.data_ptr(), bw, 0, bw, bh, 1),
                            args.steps, args.warmup)
            t_whole = timed(stream, ctx, lambda: ctx.forward_y_dev(d_plane.data_ptr(), W, 0, d_whole.data_ptr(), W, 0, W, H, 1),
                            args.steps, args.warmup)
            rec = recorded.get(name, {}).get(mode)
            print(f"\n## {name} {mode}: whole plane (srcnn_forward_y_dev) {t_whole[0]:.3f} ms [{t_whole[1]:.3f} .. {t_whole[2]:.3f}]; "
                  f"{bw}x{bh}: {t_small[0]:.3f} ms [{t_small[1]:.3f} .. {t_small[2]:.3f}]"
                  + (f", recorded in banded16_bench.json: {rec:.3f} ms ({t_small[0] / rec - 1:+.1%})" if rec else ""))
            print(f"# {'N':>2} {'rank':>4} {'rows':>5} {'ms':>9} {'min':>9} {'max':>9}")
            entry = {"model": name, "mode": mode, "width": W, "height": H, "halo_rows": R, "steps": args.steps, "warmup": args.warmup,
                     "whole_plane_ms": round(t_whole[0], 4), "whole_plane_ms_min": round(t_whole[1], 4),
                     "whole_plane_ms_max": round(t_whole[2], 4),
                     "bench_size": f"{bw}x{bh}", "bench_size_ms": round(t_small[0], 4), "bench_size_ms_min": round(t_small[1], 4),
                     "bench_size_ms_max": round(t_small[2], 4), "bench_size_ms_recorded": rec, "n": []}
            t1 = None
            for n in ns:
                ranks = []
                for k in range(n):
                    r0, r1 = S.stripe_rows(H, n, k)
                    rows = r1 - r0
                    base = d_plane.data_ptr()
                    top = base + (r0 - R) * W if k > 0 else 0          # the neighbours' edge rows, where they lie
                    bot = base + r1 * W if k < n - 1 else 0
                    if n == 1:
                        run = lambda: ctx.model_rows_dev(base, W, 0, d_out.data_ptr(), W, 0, W, H, 0, H)
                    else:
                        run = lambda: ctx.model_rows_halo_dev(base + r0 * W, W, r0, rows, top, bot, W, d_out.data_ptr(), W, 0, W, H,
                                                              r0, r1)
                    med, lo, hi = timed(stream, ctx, run, args.steps, args.warmup)
                    ranks.append({"rank": k, "rows": rows, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)})
                    print(f"  {n:>2} {k:>4} {rows:>5} {med:9.4f} {lo:9.4f} {hi:9.4f}")
                # every rank wrote its rows of d_out: the assembled plane is the whole-plane call's
                ctx.synchronize()
                if not torch.equal(d_out, d_whole):
                    raise SystemExit(f"{name} {mode} N = {n}: the assembled stripes differ from the whole plane")
                d_out.zero_()
                torch.cuda.synchronize()
                worst = max(ranks, key=lambda r: r["ms"])
                if n == 1:
                    t1 = worst["ms"]
                sides = 0 if n == 1 else 1 if n == 2 else 2
                rows = min(r["rows"] for r in ranks)
                exp_l1, exp_l2 = (rows + sides * (2 + r2)) / rows, (rows + sides * 2) / rows
                overhead = n * worst["ms"] / t1 if t1 else float("nan")
                entry["n"].append({"n": n, "ranks": ranks, "worst_ms": worst["ms"], "speedup": round(t1 / worst["ms"], 3) if t1 else None,
                                   "overhead": round(overhead, 4), "expected_l1": round(exp_l1, 4), "expected_l2": round(exp_l2, 4)})
                print(f"#  N = {n}: slowest rank {worst['ms']:.4f} ms, t(1) / t = {t1 / worst['ms']:.2f} (ideal {n}), overhead N t / t(1) = "
                      f"{overhead:.4f}; expected from the recomputed rows: layer 1 {exp_l1:.4f}, layer 2 {exp_l2:.4f}")
            results.append(entry)
    ctx.set_stream(0)
    ctx.close()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
