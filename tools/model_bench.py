"""Time the 9-1-5, 9-3-5 and 9-5-5 models (srcnn_set_model) on one GPU: device-resident planes, HIP events around each call of
srcnn_forward_y_dev on the context's stream, warm-up calls excluded.  Reports ms per plane, MPix/s and the fraction of the
f32-MFMA peak (157.3 TFLOP/s) by the algorithmic FLOP per pixel, 2 x (64*81*C + 32*64*f2^2 + 32*25*C) for C channels.

    python tools/model_bench.py [--channels 1 3] [--f2 1 3 5] [--padding replicate|zero|both] [--sizes 3840x2160 1920x1080]
                                [--mode mfma|banded16|both] [--dtype u8 f32] [--widths 64x32 128x64] [--steps 20] [--warmup 3]
                                [--json out.json]

--channels 3 times the colour models (srcnn_set_model_color) through srcnn_forward_color_dev on interleaved 3-byte pixels.

--padding both times each model and size with replicate padding, then with zero padding (srcnn_set_padding), in one process.

--mode banded16 times SRCNN_MODE_BANDED16 (layer 2 in split f16); --mode both times each configuration in SRCNN_MODE_MFMA and
then in SRCNN_MODE_BANDED16 in one process, and reports both times and their ratio (banded16 / mfma).  The fraction of peak is
of the f32 peak by the algorithmic FLOP in either mode: the figure to compare is the time.

--dtype f32 times the float image path (srcnn_forward_f32_dev: float32 planes in and out, the same pixel values as floats,
planar for 3 channels) instead of the byte entry points; --dtype u8 f32 times both in one process, the byte call first, and
reports the float times beside the byte times with their ratio (f32 / u8) per mode.

--widths N1xN2 ... times models of those filter counts (srcnn_set_model_shape; default 64x32, the models of the other loaders).
Each row then also carries the MFMAs per 32 pixels of the padded model, the FLOP they execute per pixel (128 per MFMA) and the
fraction of the peak in EXECUTED FLOP, the figure to compare rows of different widths by.  Wide models (more than 64 / 32
filters) run in SRCNN_MODE_MFMA only: for them --mode banded16 / both times the OPTION srcnn_set_wide_split16 (layer 2 in split
f16, the mode staying SRCNN_MODE_MFMA) instead of the mode, under the same keys (..._banded16, banded16_over_mfma), and the row
says so in "split_form": "wide_split16".  Both forms of a configuration run in one process, the float32 form first.
"""
import argparse
import json
import sys
from pathlib import Path

import torch  # noqa: F401  -- before the HIP library: one HIP runtime for both

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402

import srcnn_cpp_amd as S  # noqa: E402
from srcnn_cpp_amd.synth import synth_luma  # noqa: E402

PEAK_TFLOPS = 157.3


def flop_per_pixel(f2, channels=1, n1=64, n2=32):
    return 2 * (n1 * 81 * channels + n2 * n1 * f2 * f2 + n2 * 25 * channels)


def mfma_per_32_pixels(f2, channels=1, n1=64, n2=32):
    """v_mfma_f32_32x32x2_f32 instructions per 32 pixels of the banded path, widths padded to 64 / 32: layer 1 82 per channel and
    64 filters, layer 2 4 f2^2 per chunk of 8 inputs and group of 32 outputs, layer 3 one per channel and 2 maps."""
    n1p, n2p = 64 * ((n1 + 63) // 64), 32 * ((n2 + 31) // 32)
    return channels * 82 * (n1p // 64) + (n1p // 8) * f2 * f2 * 4 * (n2p // 32) + channels * (n2p // 2)


def model(f2, seed=0, n1=64, n2=32):
    rng = np.random.default_rng(seed)
    if (n1, n2) != (64, 32):
        return color_model(f2, seed, n1, n2, channels=1)
    return (rng.normal(0, 0.03, (64, 9, 9)).astype(np.float32), rng.normal(0, 1, 64).astype(np.float32),
            rng.normal(0, 0.08 / f2, (32, 64, f2, f2)).astype(np.float32), rng.normal(0, 1, 32).astype(np.float32),
            rng.normal(0, 0.02, (32, 5, 5)).astype(np.float32), 60.0)


def color_model(f2, seed=0, n1=64, n2=32, channels=3):
    rng = np.random.default_rng(seed)
    k2, k3 = np.sqrt(64.0 / n1), np.sqrt(32.0 / n2)         # other widths: the sums keep their magnitude
    return (rng.normal(0, 0.03 / np.sqrt(channels), (n1, channels, 9, 9)).astype(np.float32), rng.normal(0, 1, n1).astype(np.float32),
            rng.normal(0, 0.08 / f2 * k2, (n2, n1, f2, f2)).astype(np.float32), rng.normal(0, 1, n2).astype(np.float32),
            rng.normal(0, 0.02 * k3, (channels, n2, 5, 5)).astype(np.float32), np.full(channels, 60.0, np.float32))


def time_plane(ctx, w, h, steps, warmup, channels=1, dtype="u8"):
    if dtype == "f32":
        y = synth_luma(w, h)
        planes = np.stack([y, y[::-1], y[:, ::-1]]) if channels == 3 else y[None]
        d_src = torch.from_numpy(np.ascontiguousarray(planes).astype(np.float32)).cuda()
        run = lambda: ctx.forward_f32_dev(d_src.data_ptr(), w, w * h, 0, d_dst.data_ptr(), w, w * h, 0, w, h, 1)
    elif channels == 3:
        y = synth_luma(w, h)
        d_src = torch.from_numpy(np.ascontiguousarray(np.stack([y, y[::-1], y[:, ::-1]], axis=2))).cuda()
        run = lambda: ctx.forward_color_dev(d_src.data_ptr(), 3 * w, 0, d_dst.data_ptr(), 3 * w, 0, w, h, 1)
    else:
        d_src = torch.from_numpy(synth_luma(w, h)).cuda()
        run = lambda: ctx.forward_y_dev(d_src.data_ptr(), w, 0, d_dst.data_ptr(), w, 0, w, h, 1)
    d_dst = torch.empty_like(d_src)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
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
    finally:
        ctx.set_stream(0)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[1], choices=[1, 3])
    ap.add_argument("--f2", type=int, nargs="+", default=[3, 5], choices=[1, 3, 5])
    ap.add_argument("--padding", choices=["replicate", "zero", "both"], default="replicate")
    ap.add_argument("--mode", choices=["mfma", "banded16", "both"], default="mfma")
    ap.add_argument("--dtype", nargs="+", default=["u8"], choices=["u8", "f32"])
    ap.add_argument("--sizes", nargs="+", default=["3840x2160", "1920x1080"])
    ap.add_argument("--widths", nargs="+", default=["64x32"], help="N1xN2 filters of layers 1 and 2, up to 128x64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    paddings = ["replicate", "zero"] if args.padding == "both" else [args.padding]
    widths = [tuple(map(int, v.split("x"))) for v in args.widths]
    rows = []

    def set_form(ctx, split, wide):
        """Layer 2 in float32 or in split f16: the mode for a 64 / 32 model, the option (in SRCNN_MODE_MFMA) for a wide one."""
        ctx.set_mode(S.MODE_BANDED16 if split and not wide else S.MODE_MFMA)
        ctx.set_wide_split16(split and wide)

    with S.Context(0) as ctx:
        for channels, f2, (n1, n2) in ((c, f, v) for c in args.channels for f in args.f2 for v in widths):
            ctx.set_model(*(color_model(f2, 0, n1, n2) if channels == 3 else model(f2, 0, n1, n2)))
            wide = n1 > 64 or n2 > 32
            for size in args.sizes:
                w, h = map(int, size.split("x"))
                for padding in paddings:
                    ctx.set_padding(padding)
                    set_form(ctx, args.mode == "banded16", wide)
                    first = "u8" if "u8" in args.dtype else "f32"
                    med, best = time_plane(ctx, w, h, args.steps, args.warmup, channels, first)
                    px = w * h
                    fpp = flop_per_pixel(f2, channels, n1, n2)
                    tflops = fpp * px / (med * 1e-3) / 1e12
                    row = dict(model=f"9-{f2}-5", channels=channels, padding=padding, width=w, height=h,
                               ms_per_plane=round(med, 3), ms_min=round(best, 3),
                               mpix_per_s=round(px / (med * 1e-3) / 1e6, 1), flop_per_pixel=fpp, tflops=round(tflops, 2),
                               fraction_of_peak=round(tflops / PEAK_TFLOPS, 3), steps=args.steps, warmup=args.warmup)
                    if args.widths != ["64x32"]:
                        n_mfma = mfma_per_32_pixels(f2, channels, n1, n2)
                        row.update(widths=f"{n1}x{n2}", mfma_per_32_pixels=n_mfma, executed_flop_per_pixel=128 * n_mfma,
                                   fraction_of_peak_executed=round(128 * n_mfma * px / (med * 1e-3) / 1e12 / PEAK_TFLOPS, 3))
                    if args.dtype != ["u8"]:
                        row["dtype"] = first if len(args.dtype) == 1 else "both"
                    both_dtypes = set(args.dtype) == {"u8", "f32"}
                    if both_dtypes:
                        medf, bestf = time_plane(ctx, w, h, args.steps, args.warmup, channels, "f32")
                        row.update(ms_per_plane_f32=round(medf, 3), ms_min_f32=round(bestf, 3), f32_over_u8=round(medf / med, 3))
                        if "widths" in row:
                            row["fraction_of_peak_executed_f32"] = round(128 * n_mfma * px / (medf * 1e-3) / 1e12 / PEAK_TFLOPS, 3)
                    if args.mode != "mfma":
                        row["mode"] = "mfma" if args.mode == "both" else "banded16"
                        if wide:
                            row["split_form"] = "wide_split16"
                    if args.mode == "both":
                        set_form(ctx, True, wide)
                        med16, best16 = time_plane(ctx, w, h, args.steps, args.warmup, channels, first)
                        row.update(mode="both", ms_per_plane_banded16=round(med16, 3), ms_min_banded16=round(best16, 3),
                                   banded16_over_mfma=round(med16 / med, 3))
                        if both_dtypes:
                            med16f, best16f = time_plane(ctx, w, h, args.steps, args.warmup, channels, "f32")
                            row.update(ms_per_plane_banded16_f32=round(med16f, 3), ms_min_banded16_f32=round(best16f, 3),
                                       banded16_f32_over_u8=round(med16f / med16, 3),
                                       banded16_over_mfma_f32=round(med16f / medf, 3))
                        set_form(ctx, False, wide)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
