"""Pillow's own results for tests/pil_reference.py's shapes, inputs and filters -> tests/golden/pil_resize_golden.npz.

    python tests/golden/make_pil_resize_golden.py        (needs Pillow; made with Pillow 12.2.0)

Keys: in/<sh>x<sw>/<input> the input bytes, out/<sh>x<sw>-<dh>x<dw>/<input>/<filter> what Image.resize gave for them.
"""
import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import pil_reference as R  # noqa: E402

data = {"pillow_version": np.array(PIL.__version__)}
for sh, sw, dh, dw in R.all_shapes():
    for name, img in R.inputs(sh, sw).items():
        data[f"in/{sh}x{sw}/{name}"] = img
        for fname, f in R.FILTERS.items():
            data[f"out/{sh}x{sw}-{dh}x{dw}/{name}/{fname}"] = np.asarray(Image.fromarray(img).resize((dw, dh), Image.Resampling(f)))
np.savez_compressed(HERE / "pil_resize_golden.npz", **data)
print(f"{len(data)} arrays, {(HERE / 'pil_resize_golden.npz').stat().st_size} bytes")
