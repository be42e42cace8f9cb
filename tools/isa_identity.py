"""Do the kernels of a translation unit still compile to the instructions they had?

    python tools/isa_identity.py srcnn_spatial_kernels.hip [--rev HEAD] [--old-units A.hip B.hip ...] [--exact]

Compiles srcnn_cpp_amd/csrc/<unit> twice with `hipcc -S --cuda-device-only --offload-arch=gfx950` and the build's flags for the
unit: once as `git show <rev>:` has it (with that revision's srcnn_kernels.h and srcnn_spatial_kernels.hip, which the units
of the float and stripe forms included while they existed), once from the working tree.  Every kernel's
instruction stream and kernel descriptor (registers, LDS, private segment) is normalised -- comments and directives dropped,
kernel symbols and basic-block labels renamed -- and hashed; the check passes when every kernel of the old listing has a kernel
of the new listing with the same hash.  Kernels are matched by content, not by name: a template parameter added to a kernel
changes its mangled name and nothing else.  Prints one line per old kernel and the new kernels that have no old counterpart;
exit status 1 when an old kernel has none.  `--old a.s --new b.s` compares two listings made elsewhere.

`--old-units A B ...` is for units that were merged or split: each named unit is compiled as the revision has it (with its own
flags in the working tree's build where it is still a unit, else the flags of `unit`), and the union of their kernels is
compared with the working tree's `unit`.  `--exact` makes a new kernel without an old counterpart a failure too: the two
kernel sets are then the same, one for one.  How the four units of the banded path became one was checked with

    python tools/isa_identity.py srcnn_spatial_kernels.hip --rev <parent> --exact \
        --old-units srcnn_spatial_kernels.hip srcnn_spatial_f32.hip srcnn_spatial_rows.hip srcnn_spatial_rows_cf.hip

and how the two units of the wide forms (models of other widths) joined it with

    python tools/isa_identity.py srcnn_spatial_kernels.hip --rev <parent> --exact \
        --old-units srcnn_spatial_kernels.hip srcnn_wide_kernels.hip srcnn_wide16_kernels.hip

(79 of 79 identical; DESIGN.md 4.6 says which three lines of the layer-3 epilogue that takes).
"""
import argparse
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from srcnn_cpp_amd import build as B  # noqa: E402


def demangle(names):
    import shutil
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    try:
        out = subprocess.run([str(filt)] + list(names), check=True, capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, TypeError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(text):
    """{kernel symbol: normalised instruction stream + descriptor}"""
    out = {}
    for name, desc in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        m = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        lines = []
        for line in m.group(1).splitlines():
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
            line = re.sub(r"\b_Z\w+", "SYM", line)
            lines.append(line)
        d = [re.sub(r"\b_Z\w+", "SYM", l.strip()) for l in desc.splitlines() if l.strip()]
        out[name] = "\n".join(lines + d)
    return out


def listing(src_dir, unit, flags, out):
    subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, f"-I{src_dir}", "-S", "--cuda-device-only",
                    "-o", str(out), str(Path(src_dir) / unit)], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("unit", nargs="?", default="srcnn_spatial_kernels.hip")
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--old")
    ap.add_argument("--new")
    ap.add_argument("--old-units", nargs="+", metavar="UNIT", help="the revision's units whose kernels `unit` holds now")
    ap.add_argument("--exact", action="store_true", help="a new kernel without an old counterpart fails the check too")
    args = ap.parse_args()
    flags = [u[1] for u in B.UNITS if u[0] == args.unit and len(u) == 2][0]

    def flags_of(unit):      # a unit the build no longer has was part of `unit`: its flags
        return next((u[1] for u in B.UNITS if u[0] == unit and len(u) == 2), flags)

    old_units = args.old_units or [args.unit]
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        if args.old and args.new:
            old, new = Path(args.old).read_text(), Path(args.new).read_text()
        else:
            # the unit as the revision has it, with that revision's header and the kernel file a unit may include
            # (srcnn_image.h: what srcnn_pipeline.hip includes besides; a revision from before it has none)
            for f in dict.fromkeys((*old_units, "srcnn_kernels.h", "srcnn_spatial_kernels.hip", "srcnn_image.h")):
                shown = subprocess.run(["git", "-C", str(ROOT), "show", f"{args.rev}:srcnn_cpp_amd/csrc/{f}"],
                                       check=f != "srcnn_image.h", capture_output=True, text=True)
                if shown.returncode == 0:
                    (d / f).write_text(shown.stdout)
            old = "".join(listing(d, u, flags_of(u), d / f"old{i}.s") for i, u in enumerate(old_units))
            new = listing(B.CSRC, args.unit, flags, d / "new.s")
    ko, kn = kernels(old), kernels(new)
    names = demangle(list(ko) + list(kn))
    by_hash = {}
    for n, body in kn.items():
        by_hash.setdefault(hashlib.sha256(body.encode()).hexdigest(), []).append(n)
    bad, matched = 0, set()
    for n, body in ko.items():
        hit = by_hash.get(hashlib.sha256(body.encode()).hexdigest(), [])
        matched.update(hit)
        n_ins = sum(1 for l in body.splitlines() if not l.startswith(".") and not l.endswith(":"))
        print(f"{'identical' if hit else 'CHANGED  '}  {n_ins:6d} instructions  {names[n]}")
        bad += not hit
    for n in kn:
        if n not in matched:
            print(f"new                               {names[n]}")
    print(f"{len(ko) - bad} of {len(ko)} kernels of the old listing compile to the same instructions; "
          f"{len(kn) - len(matched)} new kernels")
    return 1 if bad or (args.exact and len(kn) != len(matched)) else 0


if __name__ == "__main__":
    sys.exit(main())
