"""The device code of the banded path's one translation unit, srcnn_spatial_kernels.hip, for the CPU tests that read it: the unit
is compiled to a listing once per process, with the build's flags, and the tests pick their family of kernels by mangled name."""
import functools
import re
import subprocess
import tempfile
from pathlib import Path

from srcnn_cpp_amd import build as B

UNIT = "srcnn_spatial_kernels.hip"
# families of layer-1 forms by what the mangled name says of Scale (NoScale or f), In (h: bytes, f: floats) and Steps...
L1 = r"spatial_l1_kernelILi\dELb[01]E(?:NS_7NoScaleE|f)"
L1_BYTES, L1_FLOATS, L1_ROWS, L1_ROWS_CF = L1 + r"hJ(?:il)?E", L1 + r"fJ(?:il)?E", L1 + r"hJNS_6L1RowsE", L1 + r"[hf]JNS_8L1RowsCFE"
# layers 2 and 3: the forms of a 64 / 32 model (an empty pack, 16 k-steps) and the wide forms of a model of other widths (a pack of
# one int: the chunk or K-step count as a kernel argument; 32 k-steps)
L2, L2H = r"spatial_l2_kernelILi\dELb[01]EJEE", r"spatial_l2h_kernelILi\dELb[01]EJEE"
L2_WIDE, L2H_WIDE = r"spatial_l2_kernelILi(\d)ELb([01])EJiEE", r"spatial_l2h_kernelILi(\d)ELb([01])EJiEE"
L3_BYTES, L3_FLOATS = r"spatial_l3_kernelILi\dELi16ELb[01]ELb[01]EhJ", r"spatial_l3_kernelILi\dELi16ELb0ELb[01]EfJ"
L3_WIDE = r"spatial_l3_kernelILi(\d)ELi32ELb([01])ELb([01])E([hf])JfffEE"


@functools.lru_cache(maxsize=None)
def listing():
    """The unit's gfx950 assembly, as text."""
    flags = [u[1] for u in B.UNITS if u[0] == UNIT and len(u) == 2][0]
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "unit.s"
        subprocess.run([B.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, f"-I{B.CSRC}", "-S", "--cuda-device-only",
                        "-o", str(out), str(B.CSRC / UNIT)], check=True, stderr=subprocess.DEVNULL)
        return out.read_text()


def kernels(pattern=""):
    """[(mangled name, kernel descriptor, instructions)] of the unit's kernels whose mangled name matches `pattern`."""
    text = listing()
    found = []
    for name, desc in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if re.search(pattern, name):
            body = re.search(rf"^{re.escape(name)}:(.*?)^\.Lfunc_end", text, re.S | re.M).group(1)
            found.append((name, desc, body))
    return found


def private_bytes(desc):
    return int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1))


def static_lds_bytes(desc):
    return int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))


def mfma_kinds(body):
    return set(re.findall(r"\b(v_mfma_\w+)", body))
