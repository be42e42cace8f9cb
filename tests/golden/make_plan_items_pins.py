#!/usr/bin/env python3
"""Pins of the work-item planner (plan_items() in srcnn_cpp_amd/csrc/srcnn_plan.cpp), taken through the tuning build's hook
srcnn_debug_plan_items (host logic, no device) BEFORE the launch path was rebuilt around one geometry decision: per case the
item count, the seam count, whether the plan keeps the seam windows of neighbouring strips apart, and a SHA-256 over the item
and seam ints.  A plan only places work -- any plan computes the same plane -- so nothing else would notice a planner that
drifts; tests/test_plan_items.py asserts that the tree reproduces every pin.
Run from the repo root:  python tests/golden/make_plan_items_pins.py [library]   (rewrites tests/golden/plan_items_pins.json)"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

N_CU, SKEW, ITEM_INTS = 256, 10, 5
SEPARATED_BIT = 1 << 30          # of the hook's n_seams output, for a caller that adds ASK_SEPARATED to wgs_per_cu
ASK_SEPARATED = 4096


def cases():
    """(n_strips, row_begin, row_end, wgs_per_cu, seams, extra_top, extra_bot)"""
    for rows in (2160, 1080, 720, 576, 64):                 # whole planes
        for n_strips in (1, 5, 10, 11, 15, 16, 30, 31):
            for per_cu in (1, 2):
                for seams in (1, 0):
                    yield (n_strips, 0, rows, per_cu, seams, 0, 0)
    for (r0, r1) in ((540, 1080), (0, 540)):                # a rank's stripe of 2160 rows, with and without its edge rows weighed
        for n_strips in (60, 61):
            for extra in (2, 0):
                yield (n_strips, r0, r1, 2, 1, extra, extra)
    yield (N_CU + 1, 0, 2160, 2, 1, 0, 0)                   # refused: more strips than compute units
    yield (5, 0, 20, 2, 1, 0, 0)                            # refused: too few rows for items of kMinRows


def plan(lib, n_strips, r0, r1, per_cu, seams, top, bot):
    fn = lib.srcnn_debug_plan_items
    fn.restype = C.c_int
    items = (C.c_int * (ITEM_INTS * 4096))()
    seam = (C.c_int * (2 * 4096))()
    n_seams = C.c_int(0)
    n = fn(N_CU, n_strips, r0, r1, SKEW, per_cu + 16 * top + 256 * bot + ASK_SEPARATED, seams, items, 4096, seam, 4096, C.byref(n_seams))
    assert n >= 0
    ns = n_seams.value & (SEPARATED_BIT - 1)
    ints = list(items[:ITEM_INTS * n]) + list(seam[:2 * ns])
    digest = hashlib.sha256(b"".join(int(v).to_bytes(4, "little", signed=True) for v in ints)).hexdigest()
    return {"n_strips": n_strips, "row_begin": r0, "row_end": r1, "wgs_per_cu": per_cu, "seams": seams, "extra_top": top,
            "extra_bot": bot, "count": n, "n_seams": ns, "separated": int(bool(n_seams.value & SEPARATED_BIT)), "sha256": digest}


def pins(lib):
    return [plan(lib, *c) for c in cases()]


if __name__ == "__main__":
    import srcnn_cpp_amd as S
    lib = C.CDLL(sys.argv[1] if len(sys.argv) > 1 else str(S.tuning_library_path()))
    out = pins(lib)
    path = ROOT / "tests" / "golden" / "plan_items_pins.json"
    path.write_text(json.dumps({"n_cu": N_CU, "skew_pct": SKEW, "cases": out}, indent=0) + "\n")
    print(f"wrote {len(out)} plans ({sum(1 for p in out if p['count'])} with items, {sum(p['separated'] for p in out)} separated)")
