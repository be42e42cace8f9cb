#!/usr/bin/env python3
"""Pins of the launch geometry (needs the GPU): for every case, what srcnn_query_plan reports and what run_strip() last launched
on the context, the latter through the tuning build's hook srcnn_debug_last_launch_plan (the six numbers of the report, then the
frames of that launch).  Taken from the library as it was BEFORE the geometry became one value (the hook patched onto it), on a
device with 256 compute units; tests/test_gpu_parity.py::test_query_plan_reports_what_was_launched runs the same cases.
Run from the repo root:  python tests/golden/make_query_plan_pins.py [library]   (rewrites tests/golden/query_plan_pins.json);
--print: the records of the tree's tuning build as one JSON line on stdout, nothing written (what the test reads)."""
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

SINGLE = [(3840, 2160), (1920, 1080), (1280, 720), (576, 576), (130, 700), (256, 96)]     # one frame, every mode below
BATCH = [(1920, 1080, n) for n in (2, 8, 31, 32)]                                         # MODE_MFMA
MODES = ("MODE_MFMA", "MODE_REFBYTES", "MODE_SPLIT16")


def records(library=None):
    import torch
    import srcnn_cpp_amd as S
    S.use_library(library or S.tuning_library_path())
    out = []
    with S.Context(0) as ctx:
        ctx.set_weights_blob(S.load_weights())
        hook = ctx._lib.srcnn_debug_last_launch_plan
        hook.restype = C.c_int

        def launched():
            got = (C.c_int * 7)()
            assert hook(ctx._h, got) == 0
            return list(got)

        def reported(w, h, n):
            q = ctx.query_plan(w, h, n)
            return [q[k] for k in ("workgroups", "seg_rows", "strips", "segments", "lds_bytes", "threads")]

        def run(call, mode, w, h, n, fn):
            fn()
            ctx.synchronize()
            out.append({"call": call, "mode": mode, "width": w, "height": h, "frames": n, "query_plan": reported(w, h, n),
                        "launch": launched()})

        for mode in MODES:
            ctx.set_mode(getattr(S, mode))
            for (w, h) in SINGLE:
                src = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
                dst = torch.zeros_like(src)
                run("forward_y_dev", mode, w, h, 1, lambda: ctx.forward_y_dev(src.data_ptr(), w, 0, dst.data_ptr(), w, 0, w, h, 1))
                if (w, h) == (576, 576):       # the whole plane as one stripe: the same geometry through the rows entry point
                    run("forward_y_rows_dev", mode, w, h, 1, lambda: ctx.forward_y_rows_dev(src.data_ptr(), w, 0, dst.data_ptr(), w, 0, w, h, 0, h))
        ctx.set_mode(S.MODE_MFMA)
        for (w, h, n) in BATCH:
            src = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
            dst = torch.zeros_like(src)
            run("forward_y_dev", "MODE_MFMA", w, h, n, lambda: ctx.forward_y_dev(src.data_ptr(), w, w * h, dst.data_ptr(), w, w * h, w, h, n))
        w = h = 576                            # the per-layer launches
        src = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        dst = torch.zeros_like(src)
        planes = torch.zeros((32, h, w), dtype=torch.float32, device="cuda")
        run("conv99x11_dev", "MODE_MFMA", w, h, 1, lambda: ctx.conv99x11_dev(src.data_ptr(), w, planes.data_ptr(), w, w * h, w, h))
        run("conv55_dev", "MODE_MFMA", w, h, 1, lambda: ctx.conv55_dev(planes.data_ptr(), w, w * h, dst.data_ptr(), w, w, h))
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return {"n_cu": n_cu, "cases": out}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--print"]
    rec = records(args[0] if args else None)
    if "--print" in sys.argv:
        print(json.dumps(rec))
    else:
        assert rec["n_cu"] == 256
        path = ROOT / "tests" / "golden" / "query_plan_pins.json"
        path.write_text(json.dumps(rec, indent=0) + "\n")
        print(f"wrote {len(rec['cases'])} cases")
