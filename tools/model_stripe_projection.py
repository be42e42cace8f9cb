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

--channels 1 3 and --dtype u8 f32 run the same for the other images the library stripes: a colour model on packed 3-byte pixels
(srcnn_model_color_rows_halo_dev against srcnn_forward_color_dev) and 1 or 3 float32 planes (srcnn_model_rows_halo_f32_dev
against srcnn_forward_f32_dev; the halo pointers carry the image's own channel pitch).  The 3840x2160 figure of those is
compared with profiles/models/f32_bench.json.  The defaults (--channels 1 --dtype u8) are the run described above.

usage: python tools/model_stripe_projection.py [--width 7680 --height 4320 --steps 20 --warmup 3] [--channels 1 3]
                                               [--dtype u8 f32] [--json out.json]
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
from model_bench import color_model, model  # noqa: E402

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


class Image:
    """One kind of image on the device -- `channels` byte channels (1: a plane, 3: packed pixels) or float32 planes -- with the
    whole-image call and the stripe calls of that kind.  Rows are `row` elements of `es` bytes; float planes lie h * w apart."""

    def __init__(self, ctx, channels, dtype, w, h):
        self.ctx, self.channels, self.f32, self.w, self.h = ctx, channels, dtype == "f32", w, h
        y = synth_luma(w, h)
        if self.f32:
            a = np.stack([y, y[::-1], y[:, ::-1]]) if channels == 3 else y[None]
            a = np.ascontiguousarray(a).astype(np.float32)
        else:
            a = np.ascontiguousarray(np.stack([y, y[::-1], y[:, ::-1]], axis=2)) if channels == 3 else y
        self.src = torch.from_numpy(a).cuda()
        self.row = w if self.f32 or channels == 1 else 3 * w
        self.es = 4 if self.f32 else 1
        self.pitch = w * h

    def like(self):
        return torch.zeros_like(self.src)

    def whole(self, dst):
        s, d, w, h, c = self.src.data_ptr(), dst.data_ptr(), self.w, self.h, self.ctx
        if self.f32:
            return lambda: c.forward_f32_dev(s, w, self.pitch, 0, d, w, self.pitch, 0, w, h, 1)
        if self.channels == 3:
            return lambda: c.forward_color_dev(s, 3 * w, 0, d, 3 * w, 0, w, h, 1)
        return lambda: c.forward_y_dev(s, w, 0, d, w, 0, w, h, 1)

    def plain(self, dst):
        """rows [0, h) through the plain stripe call"""
        s, d, w, h, c = self.src.data_ptr(), dst.data_ptr(), self.w, self.h, self.ctx
        if self.f32:
            return lambda: c.model_rows_f32_dev(s, w, self.pitch, 0, d, w, self.pitch, 0, w, h, 0, h)
        if self.channels == 3:
            return lambda: c.model_color_rows_dev(s, 3 * w, 0, d, 3 * w, 0, w, h, 0, h)
        return lambda: c.model_rows_dev(s, w, 0, d, w, 0, w, h, 0, h)

    def halo(self, dst, r0, r1, R, has_top, has_bot):
        """rows [r0, r1) through the halo form, the halo pointers aimed at the neighbouring rows of the image where they lie"""
        s, d, w, h, c, row = self.src.data_ptr(), dst.data_ptr(), self.w, self.h, self.ctx, self.row
        at = lambda y: s + y * row * self.es
        top, bot = (at(r0 - R) if has_top else 0), (at(r1) if has_bot else 0)
        if self.f32:
            return lambda: c.model_rows_halo_f32_dev(at(r0), w, self.pitch, r0, r1 - r0, top, bot, w, self.pitch, d, w, self.pitch, 0,
                                                     w, h, r0, r1)
        if self.channels == 3:
            return lambda: c.model_color_rows_halo_dev(at(r0), row, r0, r1 - r0, top, bot, row, d, row, 0, w, h, r0, r1)
        return lambda: c.model_rows_halo_dev(at(r0), w, r0, r1 - r0, top, bot, w, d, w, 0, w, h, r0, r1)


def recorded_figures(channels, dtype, bw, bh):
    """{model: {mode: ms}} of the whole-image call at bw x bh under replicate padding, from the benchmark file of the kind"""
    out = {}
    default = channels == 1 and dtype == "u8"
    keys = {"mfma": "ms_per_plane" + ("_f32" if dtype == "f32" else ""), "banded16": "ms_per_plane_banded16" + ("_f32" if dtype == "f32" else "")}
    try:
        for e in json.loads((ROOT / "profiles" / "models" / ("banded16_bench.json" if default else "f32_bench.json")).read_text()):
            if e["channels"] == channels and e["padding"] == "replicate" and (e["width"], e["height"]) == (bw, bh):
                out[e["model"]] = {m: e.get(k) for m, k in keys.items()}
    except OSError:
        pass
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns", default="1,2,4,8")
    ap.add_argument("--f2", type=int, nargs="+", default=[5, 3], choices=[3, 5])
    ap.add_argument("--modes", nargs="+", default=["mfma", "banded16"], choices=list(MODES))
    ap.add_argument("--channels", type=int, nargs="+", default=[1], choices=[1, 3])
    ap.add_argument("--dtype", nargs="+", default=["u8"], choices=["u8", "f32"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: the median of at least 20 calls")
    W, H = args.width, args.height
    ns = [int(x) for x in args.ns.split(",")]
    ctx = S.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    bw, bh = 3840, 2160                          # the size of profiles/models/banded16_bench.json and f32_bench.json
    results = []
    print(f"# tools/model_stripe_projection.py: {W}x{H} plane, one MI355X, median of {args.steps} calls after {args.warmup} warm-up calls")
    for channels, dtype in [(c, d) for c in args.channels for d in args.dtype]:
        default = channels == 1 and dtype == "u8"
        big, small = Image(ctx, channels, dtype, W, H), Image(ctx, channels, dtype, bw, bh)
        d_whole, d_out, d_small_out = big.like(), big.like(), small.like()
        recorded = recorded_figures(channels, dtype, bw, bh)
        whole_call = "srcnn_forward_f32_dev" if dtype == "f32" else "srcnn_forward_color_dev" if channels == 3 else "srcnn_forward_y_dev"
        torch.cuda.synchronize()
        for f2 in args.f2:
            r2 = (f2 - 1) // 2
            ctx.set_model(*(color_model(f2) if channels == 3 else model(f2)))
            R = ctx.model_halo_rows()
            for mode in args.modes:
                ctx.set_mode(MODES[mode])
                name = f"9-{f2}-5"
                # baselines of the same run: the whole-image call, here and at the size of the recorded benchmark
                t_small = timed(stream, ctx, small.whole(d_small_out), args.steps, args.warmup)
                t_whole = timed(stream, ctx, big.whole(d_whole), args.steps, args.warmup)
                rec = recorded.get(name, {}).get(mode)
                kind = "" if default else f" {channels} channel(s) {dtype}"
                print(f"\n## {name} {mode}{kind}: whole plane ({whole_call}) {t_whole[0]:.3f} ms [{t_whole[1]:.3f} .. {t_whole[2]:.3f}]; "
                      f"{bw}x{bh}: {t_small[0]:.3f} ms [{t_small[1]:.3f} .. {t_small[2]:.3f}]"
                      + (f", recorded in {'banded16' if default else 'f32'}_bench.json: {rec:.3f} ms ({t_small[0] / rec - 1:+.1%})" if rec else ""))
                print(f"# {'N':>2} {'rank':>4} {'rows':>5} {'ms':>9} {'min':>9} {'max':>9}")
                entry = {"model": name, "mode": mode, "channels": channels, "dtype": dtype, "width": W, "height": H, "halo_rows": R,
                         "steps": args.steps, "warmup": args.warmup,
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
                        # the neighbours' edge rows, where they lie
                        run = big.plain(d_out) if n == 1 else big.halo(d_out, r0, r1, R, k > 0, k < n - 1)
                        med, lo, hi = timed(stream, ctx, run, args.steps, args.warmup)
                        ranks.append({"rank": k, "rows": rows, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)})
                        print(f"  {n:>2} {k:>4} {rows:>5} {med:9.4f} {lo:9.4f} {hi:9.4f}")
                    # every rank wrote its rows of d_out: the assembled image is the whole-image call's
                    ctx.synchronize()
                    if not torch.equal(d_out.view(torch.uint8), d_whole.view(torch.uint8)):
                        raise SystemExit(f"{name} {mode}{kind} N = {n}: the assembled stripes differ from the whole image")
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
        del big, small, d_whole, d_out, d_small_out
        torch.cuda.empty_cache()
    ctx.set_stream(0)
    ctx.close()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
