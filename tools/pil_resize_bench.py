"""Time Pillow's resize of uint8 images (srcnn_resize_pil_image_dev) on one GPU beside the antialiased float resize
(srcnn_resize_cubic_aa_image_dev) on the same uint8 images in the same process.

    python tools/pil_resize_bench.py [--rounds 20] [--warmup 3] [--json profiles/models/pil_resize_bench.json]

One process, device-resident images, one stream, HIP events around single calls; the two calls of a row are interleaved round by
round so that clock and neighbour noise hit both alike; the figure is the median over the rounds (minimum and spread =
(max - min) / median beside it).  Rows: 1 and 3 channels, planar and H x W x C, 1920 x 1080 -> 3840 x 2160 (the tiled form),
3840 x 2160 -> 1920 x 1080 (the tiled form), 3840 x 2160 -> 1280 x 720 (ratio 3: still the tiled form) and 3840 x 2160 ->
640 x 360 (ratio 6: the general form of both calls); `form` says which form the geometry takes by the rule of srcnn_image.h.
Per row:
  `pil`   srcnn_resize_pil_image_dev, bicubic;
  `aa`    srcnn_resize_cubic_aa_image_dev on the same images (byte * 1 / 255 in, round(clamp(v * 255)) out).
Beside the times: the algorithmic bytes (source read once, destination written once; the general form moves 2 * src_h * dst_w
more per plane) and the bandwidth they imply at the median.  Before anything is timed channel 0 of the result is checked against
Pillow itself (or, without Pillow, against the numpy restatement of tests/pil_reference.py), byte for byte.
`float_vs_pillow`: on a 128 x 128 crop of the green plane of tests/golden/butterfly_bgr.npz, the share of bytes by which the
antialiased float resize, rounded to bytes by its store, differs from this call, and the largest difference.
Run the same command twice and compare.  No GPU: the tool fails; there is no CPU timing."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import srcnn_cpp_amd as S  # noqa: E402
import pil_reference as R  # noqa: E402
from resize_f32_bench import stats, timed  # noqa: E402

GEOMETRIES = [((1080, 1920), (2160, 3840)), ((2160, 3840), (1080, 1920)), ((2160, 3840), (720, 1280)), ((2160, 3840), (360, 640))]


def reference(plane, dh, dw):
    try:
        from PIL import Image
    except ImportError:
        return R.resize(plane, dh, dw, R.BICUBIC), "the numpy restatement"
    return np.asarray(Image.fromarray(plane).resize((dw, dh), Image.Resampling.BICUBIC)), "Pillow"


def images(t, hwc, scale):
    """The Image of a (C, H, W)-shaped view t of a planar or H x W x C tensor"""
    c, h, w = t.shape
    if hwc:
        return S.Image(t.data_ptr(), S.ELEM_U8, c, w * c, 1, 0, scale)
    return S.Image(t.data_ptr(), S.ELEM_U8, 1, w, h * w, 0, scale)


def alloc(c, h, w, hwc, fill=None):
    base = torch.empty((h, w, c) if hwc else (c, h, w), dtype=torch.uint8, device="cuda")
    view = base.permute(2, 0, 1) if hwc else base
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    return view


def form_of(sh, sw, dh, dw):
    ky, kx = (S.pil_taps(s, n)[1].max() if s != n else 1 for s, n in ((sh, dh), (sw, dw)))
    return "tiled" if sh <= 4 * dh and sw <= 4 * dw and max(kx, ky) <= 17 else "general"


def float_vs_pillow(ctx):
    with np.load(ROOT / "tests" / "golden" / "butterfly_bgr.npz") as z:
        crop = np.ascontiguousarray(z["src_bgr"][128:256, 128:256, 1])

    def both(x, dh, dw):
        h, w = x.shape
        src = alloc(1, h, w, False, x[None])
        a, b = alloc(1, dh, dw, False), alloc(1, dh, dw, False)
        torch.cuda.synchronize()
        ctx.resize_pil_image_dev(images(src, False, 1.0), w, h, images(a, False, 1.0), dw, dh, 1, 1, S.PIL_BICUBIC)
        ctx.resize_cubic_aa_image_dev(images(src, False, 1.0 / 255.0), w, h, images(b, False, 255.0), dw, dh, 1, 1)
        ctx.synchronize()
        return a[0].cpu().numpy(), b[0].cpu().numpy()
    rows = []
    for name, steps in (("x 2 up", [(256, 256)]), ("x 3 up", [(384, 384)]), ("/ 3 down", [(42, 42)]), ("/ 2 down then x 2 up", [(64, 64), (128, 128)])):
        p = f = crop
        for dh, dw in steps:
            p, f = both(p, dh, dw)[0], both(f, dh, dw)[1]
        d = np.abs(p.astype(int) - f.astype(int))
        rows.append({"resize": name, "share_of_bytes_that_differ": float((d != 0).mean()), "largest_difference": int(d.max())})
        print(f"float vs Pillow, {name}: {rows[-1]['share_of_bytes_that_differ']:.1%} of the bytes differ, largest difference {d.max()}")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    records = []
    with S.Context(0) as ctx:          # raises without a gfx950 GPU; the resize needs no model
        ctx.set_stream(stream.cuda_stream)
        differ = float_vs_pillow(ctx)
        for (sh, sw), (dh, dw) in GEOMETRIES:
            for channels in (1, 3):
                for hwc in (False, True):
                    x = np.random.default_rng(sh + channels).integers(0, 256, (channels, sh, sw), dtype=np.uint8)
                    src, out_p, out_a = alloc(channels, sh, sw, hwc, x), alloc(channels, dh, dw, hwc), alloc(channels, dh, dw, hwc)
                    calls = {
                        "pil": lambda: ctx.resize_pil_image_dev(images(src, hwc, 1.0), sw, sh, images(out_p, hwc, 1.0), dw, dh, channels, 1,
                                                                S.PIL_BICUBIC),
                        "aa": lambda: ctx.resize_cubic_aa_image_dev(images(src, hwc, 1.0 / 255.0), sw, sh, images(out_a, hwc, 255.0), dw, dh,
                                                                    channels, 1),
                    }
                    torch.cuda.synchronize()
                    calls["pil"]()
                    ctx.synchronize()
                    want, by = reference(x[0], dh, dw)
                    if not np.array_equal(out_p[0].cpu().numpy(), want):
                        raise SystemExit(f"{channels} channel(s) {sw}x{sh} -> {dw}x{dh}: the bytes differ from {by}'s: nothing timed")
                    ms = {k: [] for k in calls}
                    with torch.cuda.stream(stream):
                        for run in calls.values():
                            for _ in range(args.warmup):
                                run()
                        stream.synchronize()
                        for _ in range(args.rounds):
                            for name, run in calls.items():
                                ms[name].append(timed(stream, run, 1))
                    form = form_of(sh, sw, dh, dw)
                    nbytes = channels * (sh * sw + dh * dw)
                    moved = nbytes + (2 * channels * sh * dw if form == "general" else 0)
                    rec = dict(stored=f"{channels} channel(s), {'H x W x C' if hwc else 'planar'} uint8", source=f"{sw}x{sh}",
                               target=f"{dw}x{dh}", form=form, checked_against=by, algorithmic_bytes=nbytes, bytes_moved=moved,
                               **{k: stats(v) for k, v in ms.items()})
                    for k in calls:
                        rec[k]["GB_per_s"] = (moved if k == "pil" else nbytes) / rec[k]["ms_median"] / 1e6
                    rec["pil_over_aa"] = rec["pil"]["ms_median"] / rec["aa"]["ms_median"]
                    records.append(rec)
                    print(f"{rec['stored']} {rec['source']} -> {rec['target']} ({form}, {moved / 1e6:.1f} MB): " +
                          ", ".join(f"{k} {rec[k]['ms_median']:.4f} ms ({rec[k]['spread']:.1%}, {rec[k]['GB_per_s']:.0f} GB/s)" for k in calls) +
                          f"; pil / aa {rec['pil_over_aa']:.3f}", flush=True)
    result = {"tool": "tools/pil_resize_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
              "float_vs_pillow": differ, "results": records}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"pil_over_aa": [round(r["pil_over_aa"], 3) for r in records]}))


if __name__ == "__main__":
    main()
