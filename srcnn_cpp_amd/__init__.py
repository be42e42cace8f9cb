"""srcnn_cpp_amd -- MI355X-native SRCNN Y-channel conv path.

This package is a thin ctypes binding of the C ABI in ``include/srcnn_amd.h``
(``libsrcnn_amd.so``, hand-written HIP for gfx950) plus a Python restatement of
the reference's call surface for tests and the bench:

    Convolution99(src, dst, kernel, bias)                  src/srcnn.cpp:92
    Convolution11(src, dst, kernel, bias)                  src/srcnn.cpp:151
    Convolution55(src, dst, kernel, bias)                  src/srcnn.cpp:189
    Convolution99x11(src, dst, k99, b99, k11, b11)         src/srcnn.cpp:254

with the reference's argument meaning: ``dst`` is pre-allocated by the caller
and written in place, planes are 2-D numpy arrays (any row stride), feature
maps are sequences of 32 / 64 planes.  The C++ host-side mirror a reference
maintainer would use is ``include/srcnn_amd.hpp``.

There is NO CPU fallback: importing works anywhere, but every compute call
needs the HIP library and a gfx950 device and raises ``SrcnnError`` otherwise.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

__all__ = [
    "Context", "SrcnnError", "forward_y_striped_frames", "load_library", "library_path", "tuning_library_path", "use_library", "load_weights", "split_weights",
    "load_model", "split_model", "model_from_state_dict", "model_from_module", "MODEL_SIZES", "COLOR_MODEL_SIZES", "PAD_REPLICATE",
    "PAD_ZERO",
    "Convolution99", "Convolution11", "Convolution55", "Convolution99x11", "default_context",
    "MODE_MFMA", "MODE_EXACT", "MODE_SPLIT16", "MODE_REFBYTES", "MODE_REFBYTES16", "MODE_BANDED16", "FLOP_PER_PIXEL",
    "ERR_INVALID", "ERR_HIP", "ERR_NOMEM", "ERR_NODEVICE", "ERR_STATE",
    "stripe_rows", "forward_y_frames_multi", "forward_y_lanes_dev", "forward_y_striped", "forward_y_striped_dev",
    "model_striped", "model_striped_dev",
    "model_color_striped", "model_color_striped_dev", "model_striped_f32", "model_striped_f32_dev",
    "cubic_f32_taps", "cubic_aa_f32_taps", "luma_gain", "luma_for_order", "luma_bt601_studio", "LUMA_BT601",
    "ELEM_F32", "ELEM_F16", "ELEM_BF16", "ELEM_U8", "ELEM_SIZE", "Image", "image_check",
    "ChromaGrid", "chroma_grid", "chroma_taps",
    "PIL_BILINEAR", "PIL_BICUBIC", "pil_taps",
]

_PKG = Path(__file__).resolve().parent
_LIB_PATH = _PKG / "libsrcnn_amd.so"              # the product library; use_library() for another build, before the first load
_WEIGHTS_PATH = _PKG / "data" / "srcnn915_weights.f32"

MODE_MFMA = 0
MODE_EXACT = 1
MODE_SPLIT16 = 2
MODE_REFBYTES = 3          # float32 MFMA + exact fix-up of the pixels next to a truncation boundary: the reference's bytes
MODE_REFBYTES16 = 4        # opt-in: the same behind the split-f16 kernel
MODE_BANDED16 = 5          # opt-in: every whole model on the banded path with layer 2 in split f16 (9-3-5, 9-5-5, zero padding, colour)
N_WEIGHTS = 8129
# blob sizes of the 9-f2-5 models (srcnn_set_model): b1|W1|b2|W2|b3|W3 with W2 holding 2048 * f2^2 floats
MODEL_SIZES = {8129: 1, 24513: 3, 57281: 5}
# colour models (srcnn_set_model_color): blob size -> f2; b1 | W1 [64,3,9,9] | b2 | W2 | b3 [3] | W3 [3,32,5,5]
COLOR_MODEL_SIZES = {20099: 1, 36483: 3, 69251: 5}
# padding of every layer's input (srcnn_set_padding): replicate (the default, as the reference) or zero (PyTorch's nn.Conv2d default)
PAD_REPLICATE = 0
PAD_ZERO = 1
_PADDINGS = {"replicate": PAD_REPLICATE, "zero": PAD_ZERO}
# 2 x (64*81 + 32*64 + 32*25) MAC per output pixel
FLOP_PER_PIXEL = 16064
# the widest model (srcnn_set_model_shape): filters of layer 1 and of layer 2
MAX_N1, MAX_N2 = 128, 64
# luma rows {w0, w1, w2, offset} of process_rgb_f32 (srcnn_process_rgb_f32) for planes in R, G, B order: BT.601 full range
LUMA_BT601 = (0.299, 0.587, 0.114, 0.0)

# element kinds of an Image (SRCNN_ELEM_*) and their sizes in bytes
ELEM_F32, ELEM_F16, ELEM_BF16, ELEM_U8 = 0, 1, 2, 3
ELEM_SIZE = {ELEM_F32: 4, ELEM_F16: 2, ELEM_BF16: 2, ELEM_U8: 1}
# the filters of Pillow's resize (SRCNN_PIL_*: Pillow's own numbers, Image.Resampling) and the names the torch methods take
PIL_BILINEAR, PIL_BICUBIC = 2, 3
PIL_FILTERS = {"bilinear": PIL_BILINEAR, "bicubic": PIL_BICUBIC}
# what metrics_image_dev measures (SRCNN_METRIC_*): flags, and the fields of one result
METRIC_SSE, METRIC_SSIM = 1, 2
METRIC_FIELDS = ("sse", "n_px", "ssim_sum", "n_win")
# what msssim_image_dev returns per scale, the most scales it takes, and the weights of Wang, Simoncelli and Bovik for five
MSSSIM_FIELDS = ("cs_sum", "ssim_sum", "n_win")
MSSSIM_MAX_SCALES = 5
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_NODEVICE, ERR_STATE = -1, -2, -3, -4, -5      # include/srcnn_amd.h
_ERR = {-1: "invalid argument", -2: "HIP runtime error", -3: "out of memory",
        -4: "no gfx950 device", -5: "bad state"}

_u8p = C.POINTER(C.c_uint8)
_f32p = C.POINTER(C.c_float)
_f32pp = C.POINTER(_f32p)
_lib = None


class _CImage(C.Structure):      # srcnn_image
    _fields_ = [("data", C.c_void_p), ("elem", C.c_int), ("scale", C.c_float), ("px_step", C.c_size_t), ("stride", C.c_size_t),
                ("ch_pitch", C.c_size_t), ("frame_pitch", C.c_size_t)]


class SrcnnError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"srcnn error {code} ({_ERR.get(code, '?')}): {msg}")


def library_path() -> Path:
    return _LIB_PATH


def tuning_library_path() -> Path:
    """The TUNING build of the library (srcnn_cpp_amd/build.py): the product's code plus the SRCNN_DEBUG_* experiment knobs
    and the srcnn_debug_* test hooks, which the product library does not contain."""
    return _PKG / "libsrcnn_amd_tuning.so"


def use_library(path) -> None:
    """Bind this process to another build of the library (the tuning build, an A/B variant of tools/ab.sh).  Explicit and
    in-process: no environment variable redirects the binding.  Must be called before the first load."""
    global _LIB_PATH
    if _lib is not None:
        raise RuntimeError("the library is already loaded")
    _LIB_PATH = Path(path)


def load_library() -> C.CDLL:
    """dlopen libsrcnn_amd.so; fails loudly when the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise SrcnnError(-4, f"{_LIB_PATH} not built: run `python -m srcnn_cpp_amd.build` "
                             "(there is no CPU fallback)")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; a process must hold ONE
    # HIP runtime or torch tensors/streams and this library would not share a device
    # context.  Importing torch first makes the dynamic linker resolve our NEEDED
    # libamdhip64.so.7 to the copy torch already loaded (same SONAME).
    import importlib.util
    import sys
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401
    lib = C.CDLL(str(_LIB_PATH))
    sz, i, vp, imp = C.c_size_t, C.c_int, C.c_void_p, C.POINTER(_CImage)
    sigs = {
        "srcnn_abi_version": ([], i),
        "srcnn_create": ([C.POINTER(vp), i], i),
        "srcnn_destroy": ([vp], None),
        "srcnn_last_error": ([vp], C.c_char_p),
        "srcnn_set_mode": ([vp, i], i),
        "srcnn_get_mode": ([vp], i),
        "srcnn_set_stream": ([vp, vp], i),
        "srcnn_synchronize": ([vp], i),
        "srcnn_kernel_variant": ([vp], i),
        "srcnn_conv99": ([vp, _u8p, sz, _f32p, sz, i, i, _f32p, C.c_float], i),
        "srcnn_conv11": ([vp, _f32pp, sz, _f32p, sz, i, i, _f32p, C.c_float], i),
        "srcnn_conv55": ([vp, _f32pp, sz, _u8p, sz, i, i, _f32p, C.c_float], i),
        "srcnn_conv99x11": ([vp, _u8p, sz, _f32pp, sz, i, i, _f32p, _f32p, _f32p, _f32p], i),
        "srcnn_set_weights": ([vp, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float], i),
        "srcnn_set_model": ([vp, i, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float], i),
        "srcnn_get_model_f2": ([vp], i),
        "srcnn_set_padding": ([vp, i], i),
        "srcnn_get_padding": ([vp], i),
        "srcnn_set_model_color": ([vp, i, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p], i),
        "srcnn_get_model_channels": ([vp], i),
        "srcnn_set_model_shape": ([vp, i, i, i, i, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p], i),
        "srcnn_get_model_shape": ([vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)], i),
        "srcnn_set_wide_split16": ([vp, i], i),
        "srcnn_get_wide_split16": ([vp], i),
        "srcnn_forward_color": ([vp, _u8p, sz, _u8p, sz, i, i, _f32p, sz], i),
        "srcnn_forward_color_dev": ([vp, vp, sz, sz, vp, sz, sz, i, i, i, vp], i),
        "srcnn_forward_f32": ([vp, _f32p, sz, sz, _f32p, sz, sz, i, i], i),
        "srcnn_forward_f32_dev": ([vp, vp, sz, sz, sz, vp, sz, sz, sz, i, i, i], i),
        "srcnn_cubic_f32_taps": ([i, i, C.POINTER(i), _f32p], i),
        "srcnn_resize_cubic_f32": ([vp, _f32p, sz, sz, i, i, _f32p, sz, sz, i, i, i], i),
        "srcnn_resize_cubic_f32_dev": ([vp, vp, sz, sz, sz, i, i, vp, sz, sz, sz, i, i, i, i], i),
        "srcnn_cubic_aa_f32_taps": ([i, i, C.POINTER(i), C.POINTER(i), _f32p, i], i),
        "srcnn_resize_cubic_aa_f32": ([vp, _f32p, sz, sz, i, i, _f32p, sz, sz, i, i, i], i),
        "srcnn_resize_cubic_aa_f32_dev": ([vp, vp, sz, sz, sz, i, i, vp, sz, sz, sz, i, i, i, i], i),
        "srcnn_resize_cubic_aa_image_dev": ([vp, imp, i, i, imp, i, i, i, i], i),
        "srcnn_pil_taps": ([i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_int32), i], i),
        "srcnn_resize_pil_image_dev": ([vp, imp, i, i, imp, i, i, i, i, i], i),
        "srcnn_process_pil_image_dev": ([vp, imp, i, i, imp, i, i, i, i], i),
        "srcnn_process_rgb_pil_image_dev": ([vp, imp, i, i, imp, i, i, _f32p, _f32p, i, i], i),
        "srcnn_metrics_image_dev": ([vp, imp, imp, i, i, i, i, i, _f32p, C.c_double, i, vp], i),
        "srcnn_metric_psnr": ([C.c_double, C.c_double, C.c_double], C.c_double),
        "srcnn_msssim_image_dev": ([vp, imp, imp, i, i, i, i, i, _f32p, C.c_double, i, vp], i),
        "srcnn_metric_msssim": ([C.POINTER(C.c_double), i, C.POINTER(C.c_double)], C.c_double),
        "srcnn_process_f32": ([vp, _f32p, sz, sz, i, i, _f32p, sz, sz, i, i], i),
        "srcnn_process_f32_dev": ([vp, vp, sz, sz, sz, i, i, vp, sz, sz, sz, i, i, i], i),
        "srcnn_luma_gain": ([_f32p, _f32p], i),
        "srcnn_process_rgb_f32": ([vp, _f32p, sz, sz, i, i, _f32p, sz, sz, i, i, _f32p, _f32p], i),
        "srcnn_process_rgb_f32_dev": ([vp, vp, sz, sz, sz, i, i, vp, sz, sz, sz, i, i, _f32p, _f32p, i], i),
        "srcnn_image_check": ([imp, i, i, i, i, i], i),
        "srcnn_forward_image_dev": ([vp, imp, imp, i, i, i], i),
        "srcnn_resize_cubic_image_dev": ([vp, imp, i, i, imp, i, i, i, i], i),
        "srcnn_process_image_dev": ([vp, imp, i, i, imp, i, i, i], i),
        "srcnn_process_rgb_image_dev": ([vp, imp, i, i, imp, i, i, _f32p, _f32p, i], i),
        "srcnn_chroma_taps": ([i, i, i, i, C.c_double, C.c_double, C.POINTER(i), _f32p], i),
        "srcnn_set_input_range": ([vp, C.c_float], i),
        "srcnn_get_input_range": ([vp], C.c_float),
        "srcnn_forward_y": ([vp, _u8p, sz, _u8p, sz, i, i, _f32p, sz], i),
        "srcnn_forward_y_frames": ([vp, C.POINTER(_u8p), sz, C.POINTER(_u8p), sz, i, i, i], i),
        "srcnn_forward_y_dev": ([vp, vp, sz, sz, vp, sz, sz, i, i, i, vp], i),
        "srcnn_forward_y_rows_dev": ([vp, vp, sz, i, vp, sz, i, i, i, i, i], i),
        "srcnn_forward_y_rows_halo_dev": ([vp, vp, sz, i, i, vp, vp, sz, vp, sz, i, i, i, i, i], i),
        "srcnn_halo_transport": ([vp], i),
        "srcnn_forward_y_unfused_dev": ([vp, vp, sz, sz, vp, sz, sz, i, i, i, vp], i),
        "srcnn_conv99x11_dev": ([vp, vp, sz, vp, sz, sz, i, i], i),
        "srcnn_conv55_dev": ([vp, vp, sz, sz, vp, sz, i, i, vp], i),
        "srcnn_conv99x11_to_dev": ([vp, _u8p, sz, vp, sz, sz, i, i, _f32p, _f32p, _f32p, _f32p], i),
        "srcnn_conv55_from_dev": ([vp, vp, sz, sz, _u8p, sz, i, i, _f32p, C.c_float], i),
        "srcnn_dev_alloc": ([vp, sz, C.POINTER(vp)], i),
        "srcnn_dev_free": ([vp, vp], i),
        "srcnn_dev_download": ([vp, vp, vp, sz], i),
        "srcnn_dev_upload": ([vp, vp, vp, sz], i),
        "srcnn_ipc_export": ([vp, vp, C.POINTER(C.c_ubyte * 64)], i),
        "srcnn_ipc_open": ([vp, C.POINTER(C.c_ubyte * 64), C.POINTER(vp)], i),
        "srcnn_ipc_close": ([vp, vp], i),
        "srcnn_query_plan": ([vp, i, i, i, C.POINTER(i * 6)], i),
        "srcnn_fixup_stats": ([vp, C.POINTER(C.c_ulonglong * 4), C.POINTER(C.c_float), C.POINTER(C.c_float)], i),
        "srcnn_set_fixup_strict": ([vp, i], i),
        "srcnn_set_seam_deferral": ([vp, i], i),
        "srcnn_flush": ([vp], i),
        "srcnn_set_fixup_margin": ([vp, C.c_float], i),
        "srcnn_set_kernel_variant": ([vp, i], i),
        "srcnn_set_fixup_local": ([vp, C.c_float], i),
        "srcnn_fixup_local_stats": ([vp, C.POINTER(C.c_float), C.POINTER(C.c_float)], i),
        "srcnn_scaled_size": ([i, i, C.c_float, C.POINTER(i), C.POINTER(i)], i),
        "srcnn_bgr2ycrcb": ([vp, _u8p, sz, i, i, _u8p, _u8p, _u8p, sz], i),
        "srcnn_ycrcb2bgr": ([vp, _u8p, _u8p, _u8p, sz, i, i, _u8p, sz], i),
        "srcnn_resize_cubic": ([vp, _u8p, sz, i, i, _u8p, sz, i, i], i),
        "srcnn_process_bgr": ([vp, _u8p, sz, i, i, C.c_float, _u8p, sz], i),
        "srcnn_process_bgr_dev": ([vp, vp, sz, i, i, C.c_float, vp, sz], i),
        "srcnn_stripe_rows": ([i, i, i, C.POINTER(i), C.POINTER(i)], i),
        "srcnn_forward_y_frames_multi": ([C.POINTER(vp), i, C.POINTER(_u8p), sz, C.POINTER(_u8p), sz, i, i, i], i),
        "srcnn_forward_y_lanes_dev": ([C.POINTER(vp), i, C.POINTER(vp), sz, C.POINTER(vp), sz, i, i, i], i),
        "srcnn_forward_y_striped": ([C.POINTER(vp), i, _u8p, sz, _u8p, sz, i, i], i),
        "srcnn_forward_y_striped_frames": ([C.POINTER(vp), i, C.POINTER(_u8p), sz, C.POINTER(_u8p), sz, i, i, i], i),
        "srcnn_forward_y_striped_dev": ([C.POINTER(vp), i, C.POINTER(vp), sz, C.POINTER(vp), sz, i, i], i),
        "srcnn_model_halo_rows": ([vp], i),
        "srcnn_model_rows_dev": ([vp, vp, sz, i, vp, sz, i, i, i, i, i, vp], i),
        "srcnn_model_rows_halo_dev": ([vp, vp, sz, i, i, vp, vp, sz, vp, sz, i, i, i, i, i, vp], i),
        "srcnn_model_striped": ([C.POINTER(vp), i, _u8p, sz, _u8p, sz, i, i], i),
        "srcnn_model_striped_dev": ([C.POINTER(vp), i, C.POINTER(vp), sz, C.POINTER(vp), sz, i, i], i),
        "srcnn_model_color_rows_dev": ([vp, vp, sz, i, vp, sz, i, i, i, i, i, vp], i),
        "srcnn_model_color_rows_halo_dev": ([vp, vp, sz, i, i, vp, vp, sz, vp, sz, i, i, i, i, i, vp], i),
        "srcnn_model_color_striped": ([C.POINTER(vp), i, _u8p, sz, _u8p, sz, i, i], i),
        "srcnn_model_color_striped_dev": ([C.POINTER(vp), i, C.POINTER(vp), sz, C.POINTER(vp), sz, i, i], i),
        "srcnn_model_rows_f32_dev": ([vp, vp, sz, sz, i, vp, sz, sz, i, i, i, i, i], i),
        "srcnn_model_rows_halo_f32_dev": ([vp, vp, sz, sz, i, i, vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i], i),
        "srcnn_model_striped_f32": ([C.POINTER(vp), i, _f32p, sz, sz, _f32p, sz, sz, i, i], i),
        "srcnn_model_striped_f32_dev": ([C.POINTER(vp), i, C.POINTER(vp), sz, sz, C.POINTER(vp), sz, sz, i, i], i),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(lib, name)          # AttributeError if the ABI lost a symbol
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


ABI_SYMBOLS = (
    "srcnn_abi_version", "srcnn_create", "srcnn_destroy", "srcnn_last_error", "srcnn_set_mode",
    "srcnn_get_mode", "srcnn_set_stream", "srcnn_synchronize", "srcnn_kernel_variant", "srcnn_set_kernel_variant", "srcnn_conv99", "srcnn_conv11",
    "srcnn_conv55", "srcnn_conv99x11", "srcnn_set_weights", "srcnn_forward_y", "srcnn_forward_y_frames",
    "srcnn_forward_y_dev",
    "srcnn_forward_y_rows_dev", "srcnn_forward_y_rows_halo_dev", "srcnn_halo_transport", "srcnn_forward_y_unfused_dev", "srcnn_conv99x11_dev",
    "srcnn_conv55_dev", "srcnn_conv99x11_to_dev", "srcnn_conv55_from_dev", "srcnn_dev_alloc", "srcnn_dev_free",
    "srcnn_dev_download", "srcnn_dev_upload", "srcnn_ipc_export", "srcnn_ipc_open", "srcnn_ipc_close", "srcnn_query_plan", "srcnn_fixup_stats", "srcnn_set_fixup_strict", "srcnn_set_fixup_margin", "srcnn_set_fixup_local", "srcnn_fixup_local_stats", "srcnn_set_seam_deferral", "srcnn_flush", "srcnn_scaled_size", "srcnn_bgr2ycrcb", "srcnn_ycrcb2bgr",
    "srcnn_resize_cubic", "srcnn_process_bgr", "srcnn_process_bgr_dev",
    "srcnn_stripe_rows", "srcnn_forward_y_frames_multi", "srcnn_forward_y_lanes_dev", "srcnn_forward_y_striped", "srcnn_forward_y_striped_frames", "srcnn_forward_y_striped_dev",
    "srcnn_set_model", "srcnn_get_model_f2", "srcnn_set_padding", "srcnn_get_padding",
    "srcnn_set_model_color", "srcnn_get_model_channels", "srcnn_forward_color", "srcnn_forward_color_dev",
    "srcnn_set_model_shape", "srcnn_get_model_shape", "srcnn_set_wide_split16", "srcnn_get_wide_split16",
    "srcnn_forward_f32", "srcnn_forward_f32_dev", "srcnn_set_input_range", "srcnn_get_input_range",
    "srcnn_cubic_f32_taps", "srcnn_resize_cubic_f32", "srcnn_resize_cubic_f32_dev", "srcnn_process_f32", "srcnn_process_f32_dev",
    "srcnn_luma_gain", "srcnn_process_rgb_f32", "srcnn_process_rgb_f32_dev",
    "srcnn_image_check", "srcnn_forward_image_dev", "srcnn_resize_cubic_image_dev", "srcnn_process_image_dev",
    "srcnn_process_rgb_image_dev",
    "srcnn_chroma_taps",
    "srcnn_cubic_aa_f32_taps", "srcnn_resize_cubic_aa_f32", "srcnn_resize_cubic_aa_f32_dev", "srcnn_resize_cubic_aa_image_dev",
    "srcnn_metrics_image_dev", "srcnn_metric_psnr", "srcnn_msssim_image_dev", "srcnn_metric_msssim",
    "srcnn_pil_taps", "srcnn_resize_pil_image_dev", "srcnn_process_pil_image_dev", "srcnn_process_rgb_pil_image_dev",
    "srcnn_model_halo_rows", "srcnn_model_rows_dev", "srcnn_model_rows_halo_dev", "srcnn_model_striped", "srcnn_model_striped_dev",
    "srcnn_model_color_rows_dev", "srcnn_model_color_rows_halo_dev", "srcnn_model_color_striped", "srcnn_model_color_striped_dev",
    "srcnn_model_rows_f32_dev", "srcnn_model_rows_halo_f32_dev", "srcnn_model_striped_f32", "srcnn_model_striped_f32_dev",
)


def load_weights(path: Optional[Path] = None) -> np.ndarray:
    """The SRCNN 9-1-5 parameters as an 8,129-float blob in convdata.h order
    (b1|W1|b2|W2|b3|W3; provenance: oracle/dump_weights.c)."""
    blob = np.fromfile(str(path or _WEIGHTS_PATH), dtype="<f4")
    if blob.size != N_WEIGHTS:
        raise ValueError(f"weight blob has {blob.size} floats, expected {N_WEIGHTS}")
    return blob


def split_weights(blob: np.ndarray):
    """blob -> (w1[64,9,9], b1[64], w2[32,64], b2[32], w3[32,5,5], b3)."""
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    return (blob[64:5248].reshape(64, 9, 9), blob[0:64], blob[5280:7328].reshape(32, 64),
            blob[5248:5280], blob[7329:8129].reshape(32, 5, 5), float(blob[7328]))


def split_model(blob: np.ndarray):
    """A 9-1-5, 9-3-5 or 9-5-5 blob (8,129 / 24,513 / 57,281 floats, b1|W1|b2|W2|b3|W3) ->
    (w1[64,9,9], b1[64], w2, b2[32], w3[32,5,5], b3) with w2 [32,64] for f2 = 1, else [32,64,f2,f2].

    A colour blob (COLOR_MODEL_SIZES: 20,099 / 36,483 / 69,251 floats, b1|W1|b2|W2|b3[3]|W3) ->
    (w1[64,3,9,9], b1[64], w2[32,64,f2,f2], b2[32], w3[3,32,5,5], b3[3])."""
    blob = np.ascontiguousarray(blob, dtype=np.float32).ravel()
    if blob.size in COLOR_MODEL_SIZES:
        f2 = COLOR_MODEL_SIZES[blob.size]
        o2 = 64 + 15552                      # b2
        o3 = o2 + 32 + 2048 * f2 * f2        # b3
        return (blob[64:o2].reshape(64, 3, 9, 9), blob[0:64], blob[o2 + 32:o3].reshape(32, 64, f2, f2),
                blob[o2:o2 + 32], blob[o3 + 3:o3 + 2403].reshape(3, 32, 5, 5), blob[o3:o3 + 3].copy())
    f2 = MODEL_SIZES.get(blob.size)
    if f2 is None:
        raise ValueError(f"model blob has {blob.size} floats, expected one of {sorted(MODEL_SIZES)} "
                         f"(colour: {sorted(COLOR_MODEL_SIZES)})")
    if f2 == 1:
        return split_weights(blob)
    n2 = 2048 * f2 * f2
    o3 = 5280 + n2
    return (blob[64:5248].reshape(64, 9, 9), blob[0:64], blob[5280:o3].reshape(32, 64, f2, f2),
            blob[5248:5280], blob[o3 + 1:o3 + 801].reshape(32, 5, 5), float(blob[o3]))


def load_model(path) -> np.ndarray:
    """A 9-1-5, 9-3-5 or 9-5-5 model blob, 1-channel or colour, from a file (float32 little-endian, b1|W1|b2|W2|b3|W3)."""
    blob = np.fromfile(str(path), dtype="<f4")
    if blob.size not in MODEL_SIZES and blob.size not in COLOR_MODEL_SIZES:
        raise ValueError(f"model blob has {blob.size} floats, expected one of {sorted(MODEL_SIZES)} "
                         f"(colour: {sorted(COLOR_MODEL_SIZES)})")
    return blob


def model_from_state_dict(sd, input_scale: float = 255.0, image_order: Optional[str] = None):
    """A PyTorch SRCNN state dict -> (w1, b1, w2, b2, w3, b3) for Context.set_model.

    Reads conv1.weight (64,1,9,9), conv1.bias, conv2.weight (32,64,f2,f2) with f2 = 1, 3 or 5, conv2.bias,
    conv3.weight (1,32,5,5) and conv3.bias.  Other widths -- conv1.weight (n1,C,9,9), conv2.weight (n2,n1,f2,f2),
    conv3.weight (C,n2,5,5) with 1 <= n1 <= MAX_N1 = 128 and 1 <= n2 <= MAX_N2 = 64, the paper's 128 / 64 and 32 / 16 among them --
    give shaped arrays of those widths (Context.set_model reads n1 and n2 from w2's shape); ValueError for widths out of range
    and for a conv2.weight whose input count is not conv1's output count.  The library runs on 0..255 luma; a model trained on [0, 1] inputs
    (input_scale = 255, the default) gets its three biases multiplied by input_scale, which maps it exactly onto
    0..255 because ReLU is positively homogeneous (pass 1.0 for a model trained on 0..255).

    A state dict does not say how the layers pad their input.  A model built with nn.Conv2d(..., padding=k // 2) and the
    default padding_mode "zeros" -- the usual PyTorch SRCNN -- needs Context.set_padding("zero"); "replicate" (the
    context's default) is for models trained with padding_mode="replicate".  model_from_module reads the padding from an
    nn.Module.

    A colour model (num_channels = 3: conv1.weight (64,3,9,9), conv3.weight (3,32,5,5), conv3.bias (3,)) gives
    (w1[64,3,9,9], b1, w2[32,64,f2,f2], b2, w3[3,32,5,5], b3[3]) and needs image_order, the channel order of the images it
    will run on: model channel i reads byte i of a pixel.  "rgb" keeps the trained order; "bgr" (OpenCV images,
    Context.process_bgr) reverses W1's input axis and W3 / b3's output axis of a model trained on RGB.  ValueError when
    image_order is missing for a colour model, and when conv1 and conv3 disagree on the channel count.

    Every such model runs in MODE_MFMA (the default) and, opt-in, in MODE_BANDED16 (layer 2 in split f16: the same
    tolerance, a 9-5-5 model several times faster).
    """
    def arr(key, shape=None):
        if key not in sd:
            raise KeyError(f"state dict has no {key!r}")
        v = sd[key]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        v = np.asarray(v, dtype=np.float64)
        if shape is not None and v.shape != shape:
            raise ValueError(f"{key}: shape {v.shape}, expected {shape}")
        return v
    w2 = arr("conv2.weight")
    if w2.ndim != 4 or w2.shape[2] != w2.shape[3] or w2.shape[2] not in (1, 3, 5):
        raise ValueError(f"conv2.weight: shape {w2.shape}, expected (32, 64, f2, f2) with f2 in 1, 3, 5 (or (n2, n1, f2, f2) with "
                         f"n1 <= {MAX_N1}, n2 <= {MAX_N2})")
    n2, n1 = w2.shape[:2]
    if not (1 <= n1 <= MAX_N1 and 1 <= n2 <= MAX_N2):
        raise ValueError(f"conv2.weight: shape {w2.shape}: {n1} / {n2} filters, expected 1 <= n1 <= {MAX_N1} and 1 <= n2 <= {MAX_N2}")
    if arr("conv1.weight").shape[:1] != (n1,):
        raise ValueError(f"conv1.weight: shape {arr('conv1.weight').shape} and conv2.weight: shape {w2.shape}: conv2 must read "
                         "the channels conv1 writes")
    s = float(input_scale)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c_in, c_out = arr("conv1.weight").shape[1:2], arr("conv3.weight").shape[:1]
    if (n1, n2) != (64, 32):         # other widths: shaped arrays, 1 or 3 channels (Context.set_model -> srcnn_set_model_shape)
        if c_in != c_out or c_in not in ((1,), (3,)):
            raise ValueError(f"conv1 reads {c_in[0] if c_in else '?'} channels and conv3 writes {c_out[0] if c_out else '?'}: "
                             "a model has 1 channel in and out, or 3")
        ch = c_in[0]
        if ch == 3 and image_order not in ("rgb", "bgr"):
            raise ValueError(f"image_order={image_order!r}: a 3-channel model needs image_order='rgb' or 'bgr' (the channel "
                             "order of the images it will run on)")
        w1, w3, b3 = arr("conv1.weight", (n1, ch, 9, 9)), arr("conv3.weight", (ch, n2, 5, 5)), arr("conv3.bias", (ch,))
        if ch == 3 and image_order == "bgr":
            w1, w3, b3 = w1[:, ::-1], w3[::-1], b3[::-1]
        return (f32(w1), f32(arr("conv1.bias", (n1,)) * s), f32(w2), f32(arr("conv2.bias", (n2,)) * s), f32(w3), f32(b3 * s))
    if c_in == (3,) or c_out == (3,):
        if c_in != c_out:
            raise ValueError(f"conv1 reads {c_in[0] if c_in else '?'} channels and conv3 writes {c_out[0] if c_out else '?'}: "
                             "a model has 1 channel in and out, or 3")
        if image_order not in ("rgb", "bgr"):
            raise ValueError(f"image_order={image_order!r}: a 3-channel model needs image_order='rgb' or 'bgr' (the channel "
                             "order of the images it will run on)")
        w1, w3, b3 = arr("conv1.weight", (64, 3, 9, 9)), arr("conv3.weight", (3, 32, 5, 5)), arr("conv3.bias", (3,))
        if image_order == "bgr":
            w1, w3, b3 = w1[:, ::-1], w3[::-1], b3[::-1]
        return (f32(w1), f32(arr("conv1.bias", (64,)) * s), f32(w2.reshape(32, 64, w2.shape[2], w2.shape[2])),
                f32(arr("conv2.bias", (32,)) * s), f32(w3), f32(b3 * s))
    return (f32(arr("conv1.weight", (64, 1, 9, 9)).reshape(64, 9, 9)), f32(arr("conv1.bias", (64,)) * s),
            f32(w2 if w2.shape[2] > 1 else w2.reshape(32, 64)), f32(arr("conv2.bias", (32,)) * s),
            f32(arr("conv3.weight", (1, 32, 5, 5)).reshape(32, 5, 5)), float(arr("conv3.bias", (1,))[0] * s))


def model_from_module(module, input_scale: float = 255.0, image_order: Optional[str] = None):
    """A PyTorch SRCNN nn.Module with conv1, conv2 and conv3 -> (model, padding) for Context.set_model and Context.set_padding.

    model is model_from_state_dict(module.state_dict(), input_scale, image_order) (a 3-channel module needs image_order);
    padding is "zero" or "replicate", read from each conv's
    padding and padding_mode.  Every layer must pad by k // 2 in one mode: ValueError for an unpadded layer (0 or "valid"),
    for "reflect" or "circular", and for layers whose modes differ.  Both paddings run in MODE_MFMA and MODE_BANDED16.
    """
    modes = set()
    for name in ("conv1", "conv2", "conv3"):
        conv = getattr(module, name, None)
        if conv is None:
            raise ValueError(f"module has no {name}")
        k = tuple(conv.kernel_size)
        pad = conv.padding
        if isinstance(pad, str):
            if pad == "valid":
                raise ValueError(f"{name}: padding='valid' (unpadded layers are not supported)")
            pad = tuple(kk // 2 for kk in k)          # "same" with an odd kernel
        pad = tuple(pad) if isinstance(pad, (tuple, list)) else (pad, pad)
        if pad != tuple(kk // 2 for kk in k):
            raise ValueError(f"{name}: padding {pad} for kernel {k}, expected {tuple(kk // 2 for kk in k)}"
                             + (" (unpadded layers are not supported)" if pad == (0, 0) else ""))
        mode = conv.padding_mode
        if mode == "zeros":
            modes.add("zero")
        elif mode == "replicate":
            modes.add("replicate")
        else:
            raise ValueError(f"{name}: padding_mode={mode!r} (only 'zeros' and 'replicate' are supported)")
    if len(modes) != 1:
        raise ValueError(f"the layers mix padding modes {sorted(modes)}: one mode for all three layers is supported")
    return model_from_state_dict(module.state_dict(), input_scale, image_order), modes.pop()


def _plane(a, dtype, name, writable=False):
    if not isinstance(a, np.ndarray) or a.ndim != 2 or a.dtype != dtype:
        raise TypeError(f"{name}: expected a 2-D numpy array of {np.dtype(dtype).name}")
    if a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
        raise ValueError(f"{name}: rows must be contiguous (row stride may be padded)")
    if writable and not a.flags.writeable:
        raise ValueError(f"{name}: output plane is read-only")
    return a, a.strides[0] // a.itemsize


def _f32_planes(a, name, writable=False):
    """A float32 (H, W), (C, H, W) or (N, C, H, W) array as its (N, C, H, W) view: rows contiguous, the other strides whole
    floats, positive and no smaller than a row (TypeError / ValueError otherwise, before any call into the library)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim not in (2, 3, 4):
        raise TypeError(f"{name}: expected a float32 numpy array of shape (H, W), (C, H, W) or (N, C, H, W)")
    if 0 in a.shape:
        raise ValueError(f"{name}: empty array of shape {tuple(a.shape)}")
    a4 = a[(None,) * (4 - a.ndim)]
    w = a4.shape[3]
    if a4.strides[3] != 4 or (a4.shape[2] > 1 and (a4.strides[2] % 4 or a4.strides[2] < 4 * w)):
        raise ValueError(f"{name}: rows must be contiguous (row, channel and frame strides may be padded)")
    if any(a4.shape[d] > 1 and (a4.strides[d] % 4 or a4.strides[d] <= 0) for d in (0, 1)):
        raise ValueError(f"{name}: channel and frame strides must be positive multiples of 4 bytes")
    if writable and not a.flags.writeable:
        raise ValueError(f"{name}: output array is read-only")
    return a4


def _f32_image(a, name, dst_w, dst_h):
    """One float32 image (H, W) or (C, H, W) as its (C, H, W) view, and the output size of a resize as two positive ints
    (TypeError / ValueError otherwise, before any call into the library)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim not in (2, 3):
        raise TypeError(f"{name}: expected a float32 numpy array of shape (H, W) or (C, H, W)")
    a3 = _f32_planes(a, name)[0]
    for what, v in (("dst_w", dst_w), ("dst_h", dst_h)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
            raise ValueError(f"{what}: expected a positive integer, got {v!r}")
    return a3, int(dst_w), int(dst_h)


def _same_shape(name, got, want):
    """Every plane of a call has the dims the C side takes from ONE of them (the reference reads them from
    dst or src, src/srcnn.cpp:94-95, :262-263, and never checks the others): a smaller buffer would be
    overrun by the device-to-host copies, so reject it here."""
    if tuple(got) != tuple(want):
        raise ValueError(f"{name}: shape {tuple(got)} does not match the call's plane shape {tuple(want)}")


def _fp(a):
    return a.ctypes.data_as(_f32p)


def _ptr_array(planes, n, name, writable=False):
    if len(planes) != n:
        raise ValueError(f"{name}: expected {n} planes, got {len(planes)}")
    stride = None
    shape = None
    for k, p in enumerate(planes):
        _, s = _plane(p, np.float32, f"{name}[{k}]", writable)
        if stride is None:
            stride, shape = s, p.shape
        elif s != stride or p.shape != shape:
            raise ValueError(f"{name}: all planes must share shape and row stride")
    arr = (_f32p * n)(*[_fp(p) for p in planes])
    return arr, stride, shape


def _wt(a, n, name):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size != n:
        raise ValueError(f"{name}: expected {n} floats, got {a.size}")
    return a


class Context:
    """One GPU + one stream (``srcnn_ctx``).  Not thread-safe; one per thread."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.srcnn_create(C.byref(h), int(device))
        if rc != 0:
            raise SrcnnError(rc, f"srcnn_create(device={device}) -- a gfx950 GPU is required, "
                                 "there is no CPU fallback")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srcnn_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise SrcnnError(rc, self._lib.srcnn_last_error(self._h).decode())

    # -- configuration ------------------------------------------------------
    def set_mode(self, mode: int):
        """MODE_MFMA (the default), MODE_EXACT, MODE_SPLIT16, MODE_REFBYTES, MODE_REFBYTES16, or MODE_BANDED16: every whole
        model (1 or 3 channels, f2 = 1, 3, 5, either padding) on the banded path with layer 2 in split f16, the tolerance of
        MODE_MFMA; row stripes, several GPUs and the per-layer device calls are refused in it (srcnn_set_mode)."""
        self._check(self._lib.srcnn_set_mode(self._h, int(mode)))

    def set_stream(self, hip_stream: int):
        self._check(self._lib.srcnn_set_stream(self._h, C.c_void_p(int(hip_stream) or None)))
        self.stream_ptr = int(hip_stream)       # 0: the context's own stream (not visible to the caller's framework)

    def synchronize(self):
        self._check(self._lib.srcnn_synchronize(self._h))

    def kernel_variant(self) -> int:
        """0 = fast strip kernels (hardware interlock verified at create), 1 = hazard-safe kernels (srcnn_kernel_variant)."""
        return int(self._lib.srcnn_kernel_variant(self._h))

    def set_kernel_variant(self, variant: int):
        """1 = pin the hazard-safe strip kernels (same bytes, ~3 % slower), 0 = what the interlock probe allows (srcnn_set_kernel_variant)."""
        self._check(self._lib.srcnn_set_kernel_variant(self._h, int(variant)))

    def set_weights(self, w1, b1, w2, b2, w3, b3):
        w1, b1 = _wt(w1, 5184, "kernel99"), _wt(b1, 64, "bias99")
        w2, b2 = _wt(w2, 2048, "kernel11"), _wt(b2, 32, "bias11")
        w3 = _wt(w3, 800, "kernel55")
        self._check(self._lib.srcnn_set_weights(self._h, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(w3), float(b3)))

    def set_weights_blob(self, blob):
        self.set_weights(*split_weights(blob))

    def set_model(self, w1, b1, w2, b2, w3, b3):
        """A 9-1-5, 9-3-5 or 9-5-5 model (srcnn_set_model): f2 from w2's shape, (32, 64) or (32, 64, f2, f2).
        A colour model -- w1 (64, 3, 9, 9), w3 (3, 32, 5, 5), b3 of length 3 -- goes to srcnn_set_model_color.
        f2 = 3, 5 and colour models run in MODE_MFMA and, with layer 2 in split f16, in MODE_BANDED16; every other mode
        refuses them.
        Other widths (srcnn_set_model_shape): shaped arrays w1 (n1, C, 9, 9), w2 (n2, n1, f2, f2) or (n2, n1), w3 (C, n2, 5, 5)
        with n1 <= 128 and n2 <= 64 read from w2.shape[:2]; C = 1 or 3 from w1; b3 a number or C numbers.  A model padded to
        64 / 32 (the paper's 32 / 16) is an ordinary model; a wider one (128 / 64) runs whole images in MODE_MFMA only (with
        layer 2 in split f16 after set_wide_split16(True)).  Flat arrays keep meaning 64 / 32."""
        w2s = tuple(np.shape(w2))
        if len(w2s) in (2, 4) and w2s[:2] != (32, 64):
            return self._set_model_shape(w1, b1, w2, b2, w3, b3)
        if tuple(np.shape(w1)) == (64, 3, 9, 9) or tuple(np.shape(w3)) == (3, 32, 5, 5) or np.size(b3) == 3:
            return self._set_model_color(w1, b1, w2, b2, w3, b3)
        shape = tuple(np.shape(w2))
        if shape == (32, 64):
            f2 = 1
        elif len(shape) == 4 and shape[:2] == (32, 64) and shape[2] == shape[3] and shape[2] in (1, 3, 5):
            f2 = shape[2]
        else:
            raise ValueError(f"kernel2: shape {shape}, expected (32, 64) or (32, 64, f2, f2) with f2 in 1, 3, 5")
        w1, b1 = _wt(w1, 5184, "kernel99"), _wt(b1, 64, "bias99")
        w2, b2 = _wt(w2, 2048 * f2 * f2, "kernel2"), _wt(b2, 32, "bias2")
        w3 = _wt(w3, 800, "kernel55")
        self._check(self._lib.srcnn_set_model(self._h, f2, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(w3), float(b3)))

    def _set_model_color(self, w1, b1, w2, b2, w3, b3):
        for name, a, want in (("kernel1", w1, (64, 3, 9, 9)), ("kernel3", w3, (3, 32, 5, 5)), ("bias3", b3, (3,))):
            if tuple(np.shape(a)) != want:
                raise ValueError(f"{name}: shape {tuple(np.shape(a))}, expected {want} (a colour model)")
        shape = tuple(np.shape(w2))
        if len(shape) == 4 and shape[:2] == (32, 64) and shape[2] == shape[3] and shape[2] in (1, 3, 5):
            f2 = shape[2]
        elif shape == (32, 64):
            f2 = 1
        else:
            raise ValueError(f"kernel2: shape {shape}, expected (32, 64, f2, f2) with f2 in 1, 3, 5")
        w1, b1 = _wt(w1, 15552, "kernel1"), _wt(b1, 64, "bias1")
        w2, b2 = _wt(w2, 2048 * f2 * f2, "kernel2"), _wt(b2, 32, "bias2")
        w3, b3 = _wt(w3, 2400, "kernel3"), _wt(b3, 3, "bias3")
        self._check(self._lib.srcnn_set_model_color(self._h, f2, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(w3), _fp(b3)))

    def _set_model_shape(self, w1, b1, w2, b2, w3, b3):
        shape = tuple(np.shape(w2))
        if len(shape) == 2:
            shape = shape + (1, 1)
        n2, n1, f2 = shape[0], shape[1], shape[2]
        if shape[2] != shape[3] or f2 not in (1, 3, 5):
            raise ValueError(f"kernel2: shape {tuple(np.shape(w2))}, expected (n2, n1, f2, f2) with f2 in 1, 3, 5")
        if not (1 <= n1 <= MAX_N1 and 1 <= n2 <= MAX_N2):
            raise ValueError(f"kernel2: shape {tuple(np.shape(w2))}: {n1} / {n2} filters, expected 1 <= n1 <= {MAX_N1} and "
                             f"1 <= n2 <= {MAX_N2}")
        s1 = tuple(np.shape(w1))
        ch = s1[1] if len(s1) == 4 else 1
        if ch not in (1, 3) or s1 not in ((n1, ch, 9, 9), (n1, 9, 9)):
            raise ValueError(f"kernel1: shape {s1}, expected ({n1}, C, 9, 9) with C = 1 or 3 (kernel2 reads {n1} channels)")
        if tuple(np.shape(w3)) not in ((ch, n2, 5, 5),) + (((n2, 5, 5),) if ch == 1 else ()):
            raise ValueError(f"kernel3: shape {tuple(np.shape(w3))}, expected ({ch}, {n2}, 5, 5)")
        w1, b1 = _wt(w1, n1 * ch * 81, "kernel1"), _wt(b1, n1, "bias1")
        w2, b2 = _wt(w2, n2 * n1 * f2 * f2, "kernel2"), _wt(b2, n2, "bias2")
        w3, b3 = _wt(w3, ch * n2 * 25, "kernel3"), _wt(b3, ch, "bias3")
        self._check(self._lib.srcnn_set_model_shape(self._h, ch, n1, f2, n2, _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(w3), _fp(b3)))

    def model_shape(self):
        """(channels, n1, f2, n2) of the loaded model (srcnn_get_model_shape): the filters as given to set_model, 64 / 32 for
        every model of those widths."""
        v = [C.c_int(0) for _ in range(4)]
        self._check(self._lib.srcnn_get_model_shape(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def set_wide_split16(self, on: bool):
        """Layer 2 of a model wider than 64 / 32 in split f16 (srcnn_set_wide_split16): off by default.  On, MODE_MFMA runs such a
        model with the arithmetic MODE_BANDED16 gives the 64 / 32 models -- layer 1 writes f16 (hi, lo) pairs, layer 2 runs on the
        f16 matrix pipe, layer 3 is unchanged -- within the tolerance of the float32 form and several times faster for f2 = 3, 5.
        A setting of the context like the padding: it survives set_model, a narrow model ignores it, and every other mode still
        refuses a wide model.  Float calls scale by set_input_range(), byte calls by 255.  A model the split cannot scale
        (non-finite weights in layers 1-2) is refused at the first call with the option on, and runs with it off."""
        self._check(self._lib.srcnn_set_wide_split16(self._h, 1 if on else 0))

    def wide_split16(self) -> bool:
        """srcnn_get_wide_split16."""
        return int(self._lib.srcnn_get_wide_split16(self._h)) == 1

    def set_model_blob(self, blob):
        self.set_model(*split_model(blob))

    def model_channels(self) -> int:
        """3 while a colour model (srcnn_set_model_color) is loaded, else 1."""
        return int(self._lib.srcnn_get_model_channels(self._h))

    def forward_color(self, img, dst=None, preclamp=None):
        """A colour model on an HxWx3 uint8 image of packed pixels (row stride may be padded); model channel i reads and
        writes byte i of a pixel.  preclamp: an HxWx3 float32 array for the values before truncation, or None."""
        img, ss = _image(img, "img")
        h, w, _ = img.shape
        if dst is None:
            dst = np.empty((h, w, 3), np.uint8)
        dst, ds = _image(dst, "dst", True)
        _same_shape("dst", dst.shape, img.shape)
        pp, ps = None, 0
        if preclamp is not None:
            if not isinstance(preclamp, np.ndarray) or preclamp.dtype != np.float32 or preclamp.ndim != 3:
                raise TypeError("preclamp: expected an HxWx3 float32 array")
            _same_shape("preclamp", preclamp.shape, img.shape)
            if preclamp.strides[2] != 4 or preclamp.strides[1] != 12 or preclamp.strides[0] % 4 or not preclamp.flags.writeable:
                raise ValueError("preclamp: pixels must be packed and writeable (row stride may be padded)")
            pp, ps = _fp(preclamp), preclamp.strides[0] // 4
        self._check(self._lib.srcnn_forward_color(self._h, img.ctypes.data_as(_u8p), ss, dst.ctypes.data_as(_u8p), ds, w, h,
                                                  pp, ps))
        return dst

    def forward_color_dev(self, d_src, src_stride, src_frame_pitch, d_dst, dst_stride, dst_frame_pitch,
                          width, height, n_frames=1, d_preclamp=0):
        """srcnn_forward_color_dev: strides and frame pitches in bytes; d_preclamp (floats) uses the dst strides."""
        self._check(self._lib.srcnn_forward_color_dev(self._h, d_src, src_stride, src_frame_pitch, d_dst, dst_stride,
                                                      dst_frame_pitch, width, height, n_frames, d_preclamp or None))

    def forward_f32(self, x, out=None):
        """The loaded whole model on float32 planes in the model's own units, the value before truncation out (srcnn_forward_f32):
        x is (H, W), (C, H, W) or (N, C, H, W) with C the model's channel count ((H, W): a 1-channel model), rows contiguous,
        row / channel / frame strides free; returns an array of the same shape (out, or a new one).  MODE_MFMA and
        MODE_BANDED16 only; inputs must be finite (and within set_input_range() in MODE_BANDED16)."""
        x4 = _f32_planes(x, "x")
        if out is None:
            out = np.empty(x.shape, np.float32)
        o4 = _f32_planes(out, "out", True)
        _same_shape("out", out.shape, x.shape)
        n, c, h, w = x4.shape
        if c not in (1, 3):
            raise ValueError(f"x: shape {tuple(x.shape)}: a model has 1 channel or 3")
        channels = self.model_channels()
        if c != channels:
            raise ValueError(f"x: shape {tuple(x.shape)} for a model of {channels} channel(s): expected (N, {channels}, H, W), "
                             f"({channels}, H, W)" + (" or (H, W)" if channels == 1 else ""))
        stride = lambda a4: a4.strides[2] // 4 if h > 1 else w
        for k in range(n):
            self._check(self._lib.srcnn_forward_f32(self._h, _fp(x4[k]), stride(x4), x4.strides[1] // 4 if c > 1 else 0, _fp(o4[k]),
                                                    stride(o4), o4.strides[1] // 4 if c > 1 else 0, w, h))
        return out

    def forward_f32_dev(self, d_src, src_stride, src_ch_pitch, src_frame_pitch, d_dst, dst_stride, dst_ch_pitch,
                        dst_frame_pitch, width, height, n_frames=1):
        """srcnn_forward_f32_dev: device addresses of float32 planes, strides and pitches in floats, asynchronous on the
        context's stream; the channel pitches are ignored for a 1-channel model."""
        self._check(self._lib.srcnn_forward_f32_dev(self._h, d_src, src_stride, src_ch_pitch, src_frame_pitch, d_dst, dst_stride,
                                                    dst_ch_pitch, dst_frame_pitch, width, height, n_frames))

    def resize_cubic_f32(self, x, dst_w, dst_h):
        """Bicubic resize of float32 planes as torch.nn.functional.interpolate(mode="bicubic", align_corners=False) defines it
        (srcnn_resize_cubic_f32): x is (H, W) or (C, H, W), rows contiguous, row and channel strides free; returns a new
        (dst_h, dst_w) or (C, dst_h, dst_w) array.  Needs no model and runs in every mode."""
        x3, dst_w, dst_h = _f32_image(x, "x", dst_w, dst_h)
        c, h, w = x3.shape
        out = np.empty((c, dst_h, dst_w), np.float32)
        self._check(self._lib.srcnn_resize_cubic_f32(self._h, _fp(x3), x3.strides[1] // 4 if h > 1 else w,
                                                     x3.strides[0] // 4 if c > 1 else 0, w, h, _fp(out), dst_w, dst_w * dst_h,
                                                     dst_w, dst_h, c))
        return out if x.ndim == 3 else out[0]

    def resize_cubic_f32_dev(self, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst, dst_stride,
                             dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, channels=1, n_frames=1):
        """srcnn_resize_cubic_f32_dev: device addresses of float32 planes, strides and pitches in floats, `channels` planes of
        n_frames frames in one launch, asynchronous on the context's stream."""
        self._check(self._lib.srcnn_resize_cubic_f32_dev(self._h, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h,
                                                         d_dst, dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, channels,
                                                         n_frames))

    def resize_cubic_aa_f32(self, x, dst_w, dst_h):
        """Antialiased bicubic resize of float32 planes as torch.nn.functional.interpolate(mode="bicubic", align_corners=False,
        antialias=True) defines it (srcnn_resize_cubic_aa_f32): the resize that shrinks without aliasing.  x, the result and the
        sizes as resize_cubic_f32 takes them.  Needs no model and runs in every mode."""
        x3, dst_w, dst_h = _f32_image(x, "x", dst_w, dst_h)
        c, h, w = x3.shape
        out = np.empty((c, dst_h, dst_w), np.float32)
        self._check(self._lib.srcnn_resize_cubic_aa_f32(self._h, _fp(x3), x3.strides[1] // 4 if h > 1 else w,
                                                        x3.strides[0] // 4 if c > 1 else 0, w, h, _fp(out), dst_w, dst_w * dst_h,
                                                        dst_w, dst_h, c))
        return out if x.ndim == 3 else out[0]

    def resize_cubic_aa_f32_dev(self, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst, dst_stride,
                                dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, channels=1, n_frames=1):
        """srcnn_resize_cubic_aa_f32_dev: the arguments of resize_cubic_f32_dev, the antialiased arithmetic."""
        self._check(self._lib.srcnn_resize_cubic_aa_f32_dev(self._h, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h,
                                                            d_dst, dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, channels,
                                                            n_frames))

    def process_f32(self, x, dst_w, dst_h):
        """resize_cubic_f32 to (dst_h, dst_w), then the loaded whole model on the result (srcnn_process_f32): x is (C, H, W)
        with C the model's channel count, or (H, W) for a 1-channel model; returns an array of the resized shape.  MODE_MFMA
        and MODE_BANDED16 only, like forward_f32."""
        x3, dst_w, dst_h = _f32_image(x, "x", dst_w, dst_h)
        c, h, w = x3.shape
        channels = self.model_channels()
        if c != channels:
            raise ValueError(f"x: shape {tuple(x.shape)} for a model of {channels} channel(s): expected ({channels}, H, W)"
                             + (" or (H, W)" if channels == 1 else ""))
        out = np.empty((c, dst_h, dst_w), np.float32)
        self._check(self._lib.srcnn_process_f32(self._h, _fp(x3), x3.strides[1] // 4 if h > 1 else w,
                                                x3.strides[0] // 4 if c > 1 else 0, w, h, _fp(out), dst_w, dst_w * dst_h, dst_w,
                                                dst_h))
        return out if x.ndim == 3 else out[0]

    def process_f32_dev(self, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst, dst_stride, dst_ch_pitch,
                        dst_frame_pitch, dst_w, dst_h, n_frames=1):
        """srcnn_process_f32_dev: resize + model on device memory, the channel count from the loaded model, asynchronous on
        the context's stream; equals resize_cubic_f32_dev followed by forward_f32_dev bit for bit."""
        self._check(self._lib.srcnn_process_f32_dev(self._h, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst,
                                                    dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, n_frames))

    def process_rgb_f32(self, x, dst_w, dst_h, luma=LUMA_BT601, clamp=None):
        """A 3-plane float32 image through the loaded 1-CHANNEL model (srcnn_process_rgb_f32): x is (3, H, W), rows contiguous;
        returns (3, dst_h, dst_w) = resize(x_c) + g (model(Yup) - Yup) per plane, Yup the resize of the luma
        ((w0 x0 + w1 x1) + w2 x2) + offset, g = luma_gain(luma); clamp = (lo, hi) bounds the result.  Never shrinks; the same
        size is allowed.  MODE_MFMA and MODE_BANDED16 only (set_input_range must then bound |Y|)."""
        x3, dst_w, dst_h = _f32_image(x, "x", dst_w, dst_h)
        if x.ndim != 3 or x3.shape[0] != 3:
            raise ValueError(f"x: shape {tuple(x.shape)}: expected (3, H, W)")
        _, h, w = x3.shape
        _not_shrinking(w, h, dst_w, dst_h)
        luma4, clamp2 = _luma4(luma), _clamp2(clamp)
        out = np.empty((3, dst_h, dst_w), np.float32)
        self._check(self._lib.srcnn_process_rgb_f32(self._h, _fp(x3), x3.strides[1] // 4 if h > 1 else w, x3.strides[0] // 4, w, h,
                                                    _fp(out), dst_w, dst_w * dst_h, dst_w, dst_h, luma4, clamp2))
        return out

    def process_rgb_f32_dev(self, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst, dst_stride, dst_ch_pitch,
                            dst_frame_pitch, dst_w, dst_h, luma=LUMA_BT601, clamp=None, n_frames=1):
        """srcnn_process_rgb_f32_dev: device addresses of 3 float32 planes each side, strides and pitches in floats,
        asynchronous on the context's stream; equals resize_cubic_f32_dev of the planes and of the luma, forward_f32_dev and
        three float32 operations, bit for bit."""
        _not_shrinking(src_w, src_h, dst_w, dst_h)
        luma4, clamp2 = _luma4(luma), _clamp2(clamp)
        self._check(self._lib.srcnn_process_rgb_f32_dev(self._h, d_src, src_stride, src_ch_pitch, src_frame_pitch, src_w, src_h, d_dst,
                                                        dst_stride, dst_ch_pitch, dst_frame_pitch, dst_w, dst_h, luma4, clamp2,
                                                        n_frames))

    def forward_image_dev(self, src: "Image", dst: "Image", width, height, n_frames=1):
        """srcnn_forward_image_dev: forward_f32_dev on images as they are stored (Image: element kind, pixel step, strides);
        equals store(forward_f32_dev(load(src))) bit for bit, asynchronous on the context's stream."""
        self._check(self._lib.srcnn_forward_image_dev(self._h, C.byref(src.c()), C.byref(dst.c()), width, height, n_frames))

    def resize_cubic_image_dev(self, src: "Image", src_w, src_h, dst: "Image", dst_w, dst_h, channels, n_frames=1):
        """srcnn_resize_cubic_image_dev: resize_cubic_f32_dev on stored images; the same size is a pure format conversion."""
        self._check(self._lib.srcnn_resize_cubic_image_dev(self._h, C.byref(src.c()), src_w, src_h, C.byref(dst.c()), dst_w, dst_h,
                                                           channels, n_frames))

    def resize_cubic_aa_image_dev(self, src: "Image", src_w, src_h, dst: "Image", dst_w, dst_h, channels, n_frames=1):
        """srcnn_resize_cubic_aa_image_dev: resize_cubic_aa_f32_dev on stored images, read and written in their own format."""
        self._check(self._lib.srcnn_resize_cubic_aa_image_dev(self._h, C.byref(src.c()), src_w, src_h, C.byref(dst.c()), dst_w,
                                                              dst_h, channels, n_frames))

    def resize_pil_image_dev(self, src: "Image", src_w, src_h, dst: "Image", dst_w, dst_h, channels, n_frames=1, filter=PIL_BICUBIC):
        """srcnn_resize_pil_image_dev: Pillow's Image.resize of uint8 pictures, byte for byte (filter: PIL_BILINEAR or
        PIL_BICUBIC), on two ELEM_U8 images where they lie; any sizes, no model needed, asynchronous on the context's stream."""
        self._check(self._lib.srcnn_resize_pil_image_dev(self._h, C.byref(src.c()), src_w, src_h, C.byref(dst.c()), dst_w, dst_h,
                                                         channels, n_frames, int(filter)))

    def process_pil_image_dev(self, src: "Image", src_w, src_h, dst: "Image", dst_w, dst_h, n_frames=1, filter=PIL_BICUBIC):
        """srcnn_process_pil_image_dev: resize_pil_image_dev of the model's channels into a uint8 image of the context that
        carries src's scale, then forward_image_dev from it into dst (any element kind); never shrinks."""
        self._check(self._lib.srcnn_process_pil_image_dev(self._h, C.byref(src.c()), src_w, src_h, C.byref(dst.c()), dst_w, dst_h,
                                                          n_frames, int(filter)))

    def process_rgb_pil_image_dev(self, src: "Image", src_w, src_h, dst: "Image", dst_w, dst_h, luma=LUMA_BT601, clamp=None,
                                  n_frames=1, filter=PIL_BICUBIC):
        """srcnn_process_rgb_pil_image_dev: resize_pil_image_dev of 3 channels, then process_rgb_image_dev at the same size."""
        _not_shrinking(src_w, src_h, dst_w, dst_h)
        luma4, clamp2 = _luma4(luma), _clamp2(clamp)
        self._check(self._lib.srcnn_process_rgb_pil_image_dev(self._h, C.byref(src.c()), src_w, src_h, C.byref(dst.c()), dst_w,
                                                              dst_h, luma4, clamp2, n_frames, int(filter)))

    def metrics_image_dev(self, a: "Image", b: "Image", width, height, channels, n_frames, border, luma, data_range, flags, d_out):
        """srcnn_metrics_image_dev: {sse, n_px, ssim_sum, n_win} per (frame, result) of two stored images, float64 after the
        load, into device memory at d_out (n_frames * P * 4 doubles; P = 1 with a luma, else channels).  luma: None or
        (w0, w1, w2, offset); flags: METRIC_SSE | METRIC_SSIM.  Asynchronous on the context's stream; needs no model."""
        luma4, ca, cb = _metric_luma4(luma), a.c(), b.c()      # refused here, before the library is reached
        self._check(self._lib.srcnn_metrics_image_dev(self._h, C.byref(ca), C.byref(cb), int(width), int(height), int(channels),
                                                      int(n_frames), int(border), luma4, float(data_range), int(flags), d_out))

    def msssim_image_dev(self, a: "Image", b: "Image", width, height, channels, n_frames, border, luma, data_range, n_scales, d_out):
        """srcnn_msssim_image_dev: {cs_sum, ssim_sum, n_win} per (frame, result, scale) of two stored images, float64 after the
        load, into device memory at d_out (n_frames * P * n_scales * 3 doubles; P = 1 with a luma, else channels).  The border is
        shaved at scale 0; scale j + 1 is the 2 x 2 mean of scale j; n_scales: 1 .. 5, and the region at least
        10 * 2^(n_scales - 1) + 1 on a side.  Asynchronous on the context's stream; needs no model."""
        luma4, ca, cb = _metric_luma4(luma), a.c(), b.c()      # refused here, before the library is reached
        self._check(self._lib.srcnn_msssim_image_dev(self._h, C.byref(ca), C.byref(cb), int(width), int(height), int(channels),
                                                     int(n_frames), int(border), luma4, float(data_range), int(n_scales), d_out))

    def process_image_dev(self, src: "Image", src_w, src_h, dst: "Image", dst_w, dst_h, n_frames=1):
        """srcnn_process_image_dev: process_f32_dev (resize + model) on stored images."""
        self._check(self._lib.srcnn_process_image_dev(self._h, C.byref(src.c()), src_w, src_h, C.byref(dst.c()), dst_w, dst_h,
                                                      n_frames))

    def process_rgb_image_dev(self, src: "Image", src_w, src_h, dst: "Image", dst_w, dst_h, luma=LUMA_BT601, clamp=None, n_frames=1):
        """srcnn_process_rgb_image_dev: process_rgb_f32_dev (a 3-channel image through the loaded 1-channel model) on stored
        images; the clamp applies in float32, ahead of the store."""
        _not_shrinking(src_w, src_h, dst_w, dst_h)
        luma4, clamp2 = _luma4(luma), _clamp2(clamp)
        self._check(self._lib.srcnn_process_rgb_image_dev(self._h, C.byref(src.c()), src_w, src_h, C.byref(dst.c()), dst_w, dst_h,
                                                          luma4, clamp2, n_frames))

    def set_input_range(self, r: float):
        """The largest |input| of a float call (srcnn_set_input_range): 255 by default, 1.0 for [0, 1] data.  A setting of the
        context; only MODE_BANDED16 reads it, and only in forward_f32 / forward_f32_dev."""
        self._check(self._lib.srcnn_set_input_range(self._h, float(r)))

    def input_range(self) -> float:
        """srcnn_get_input_range."""
        return float(self._lib.srcnn_get_input_range(self._h))

    def model_f2(self) -> int:
        """f2 of the loaded model: 1 (9-1-5, also after set_weights), 3 or 5."""
        return int(self._lib.srcnn_get_model_f2(self._h))

    def set_padding(self, padding):
        """"zero" (PyTorch's nn.Conv2d(..., padding=k // 2)) or "replicate" (the default), or PAD_ZERO / PAD_REPLICATE
        (srcnn_set_padding).  A setting of the context: it applies to the model loaded before or after it.  Zero padding
        runs in MODE_MFMA and MODE_BANDED16."""
        if isinstance(padding, str):
            if padding not in _PADDINGS:
                raise ValueError(f"padding {padding!r}: expected 'zero' or 'replicate'")
            padding = _PADDINGS[padding]
        self._check(self._lib.srcnn_set_padding(self._h, int(padding)))

    def padding(self) -> str:
        """"replicate" or "zero" (srcnn_get_padding)."""
        v = int(self._lib.srcnn_get_padding(self._h))
        return {PAD_REPLICATE: "replicate", PAD_ZERO: "zero"}[v]

    def query_plan(self, width, height, n_frames=1):
        out = (C.c_int * 6)()
        self._check(self._lib.srcnn_query_plan(self._h, width, height, n_frames, C.byref(out)))
        return dict(workgroups=out[0], seg_rows=out[1], strips=out[2], segments=out[3],
                    lds_bytes=out[4], threads=out[5])

    # -- the reference call surface (host buffers, dst written in place) ----
    def conv99(self, src, dst, kernel, bias):
        src, ss = _plane(src, np.uint8, "src")
        dst, ds = _plane(dst, np.float32, "dst", True)
        k = _wt(kernel, 81, "kernel")
        h, w = dst.shape                       # dims come from dst: src/srcnn.cpp:94-95
        _same_shape("src", src.shape, dst.shape)
        self._check(self._lib.srcnn_conv99(self._h, src.ctypes.data_as(_u8p), ss, _fp(dst), ds, w, h,
                                           _fp(k), float(bias)))

    def conv11(self, src, dst, kernel, bias):
        arr, ss, shape = _ptr_array(src, 64, "src")
        dst, ds = _plane(dst, np.float32, "dst", True)
        k = _wt(kernel, 64, "kernel")
        h, w = dst.shape
        _same_shape("src planes", shape, dst.shape)
        self._check(self._lib.srcnn_conv11(self._h, arr, ss, _fp(dst), ds, w, h, _fp(k), float(bias)))

    def conv55(self, src, dst, kernel, bias):
        arr, ss, shape = _ptr_array(src, 32, "src")
        dst, ds = _plane(dst, np.uint8, "dst", True)
        k = _wt(kernel, 800, "kernel")
        h, w = dst.shape
        _same_shape("src planes", shape, dst.shape)
        self._check(self._lib.srcnn_conv55(self._h, arr, ss, dst.ctypes.data_as(_u8p), ds, w, h,
                                           _fp(k), float(bias)))

    def conv99x11(self, src, dst, k99, b99, k11, b11):
        src, ss = _plane(src, np.uint8, "src")
        arr, ds, shape = _ptr_array(dst, 32, "dst", True)
        k99, b99 = _wt(k99, 5184, "kernel99"), _wt(b99, 64, "bias99")
        k11, b11 = _wt(k11, 2048, "kernel11"), _wt(b11, 32, "bias11")
        h, w = src.shape                       # dims come from src: src/srcnn.cpp:262-263
        _same_shape("dst planes", shape, src.shape)
        self._check(self._lib.srcnn_conv99x11(self._h, src.ctypes.data_as(_u8p), ss, arr, ds, w, h,
                                              _fp(k99), _fp(b99), _fp(k11), _fp(b11)))

    def fixup_stats(self):
        """SRCNN_MODE_REFBYTES counters since the context was created (srcnn_fixup_stats; synchronises)."""
        out, delta, dev = (C.c_ulonglong * 4)(), C.c_float(), C.c_float()
        self._check(self._lib.srcnn_fixup_stats(self._h, C.byref(out), C.byref(delta), C.byref(dev)))
        return {"scattered_pixels": int(out[0]), "dense_tiles": int(out[1]), "bytes_changed": int(out[2]),
                "exact_reruns": int(out[3]), "delta": float(delta.value), "max_dev": float(dev.value)}

    def set_fixup_strict(self, on: bool = True):
        """SRCNN_MODE_REFBYTES: redo a launch in the reference's arithmetic on every pixel when its monitored deviation exceeds
        delta / 2 -- on the device, no host read; ON by default."""
        self._check(self._lib.srcnn_set_fixup_strict(self._h, int(bool(on))))

    def set_seam_deferral(self, on: bool = True):
        """Fused float32 launches queued back to back: the seam blocks of a launch ride behind the NEXT launch's work items instead
        of a launch of their own (srcnn_set_seam_deferral).  The last launch's output is complete only after ``flush()`` or any
        other call on the context."""
        self._check(self._lib.srcnn_set_seam_deferral(self._h, int(bool(on))))

    def flush(self):
        """Queue pending deferred seam work on its stream (srcnn_flush; does not wait)."""
        self._check(self._lib.srcnn_flush(self._h))

    def set_fixup_margin(self, factor: float):
        """SRCNN_MODE_REFBYTES: delta = factor x (noise scale of the model) + absolute term; default 4."""
        self._check(self._lib.srcnn_set_fixup_margin(self._h, float(factor)))

    def set_fixup_local(self, k_local: float):
        """SRCNN_MODE_REFBYTES: the per-pixel flag threshold min(delta, margin * k_local * 2^-24 * S1(x) + abs); 0 = the one
        global threshold of rounds 3-5 (srcnn_set_fixup_local)."""
        self._check(self._lib.srcnn_set_fixup_local(self._h, float(k_local)))

    def fixup_local_stats(self):
        """(k in effect, largest |v_mfma - v_reference| / the pixel's own threshold met so far) -- srcnn_fixup_local_stats."""
        k, r = C.c_float(), C.c_float()
        self._check(self._lib.srcnn_fixup_local_stats(self._h, C.byref(k), C.byref(r)))
        return float(k.value), float(r.value)

    # the two reference calls with the 32-plane map kept in device memory between them (include/srcnn_amd.h)
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._lib.srcnn_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, d_ptr: int):
        self._check(self._lib.srcnn_dev_free(self._h, d_ptr))

    def dev_download(self, dst: np.ndarray, d_src: int):
        if not (isinstance(dst, np.ndarray) and dst.flags.c_contiguous and dst.flags.writeable):
            raise ValueError("dst: expected a writeable C-contiguous numpy array")
        self._check(self._lib.srcnn_dev_download(self._h, dst.ctypes.data_as(C.c_void_p), d_src, dst.nbytes))
        return dst

    def dev_upload(self, d_dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        self._check(self._lib.srcnn_dev_upload(self._h, d_dst, src.ctypes.data_as(C.c_void_p), src.nbytes))

    # device memory shared with the other ranks of the node (srcnn_ipc_*): a 64-byte handle out, a device address in
    def ipc_export(self, d_ptr: int) -> bytes:
        h = (C.c_ubyte * 64)()
        self._check(self._lib.srcnn_ipc_export(self._h, d_ptr, C.byref(h)))
        return bytes(h)

    def ipc_open(self, handle: bytes) -> int:
        if len(handle) != 64:
            raise ValueError("an IPC handle is 64 bytes")
        h = (C.c_ubyte * 64).from_buffer_copy(handle)
        p = C.c_void_p()
        self._check(self._lib.srcnn_ipc_open(self._h, C.byref(h), C.byref(p)))
        return p.value

    def ipc_close(self, d_ptr: int):
        self._check(self._lib.srcnn_ipc_close(self._h, d_ptr))

    def conv99x11_to_dev(self, src, d_planes, plane_stride, plane_pitch, k99, b99, k11, b11):
        src, ss = _plane(src, np.uint8, "src")
        k99, b99 = _wt(k99, 5184, "kernel99"), _wt(b99, 64, "bias99")
        k11, b11 = _wt(k11, 2048, "kernel11"), _wt(b11, 32, "bias11")
        h, w = src.shape
        self._check(self._lib.srcnn_conv99x11_to_dev(self._h, src.ctypes.data_as(_u8p), ss, d_planes, plane_stride, plane_pitch,
                                                     w, h, _fp(k99), _fp(b99), _fp(k11), _fp(b11)))

    def conv55_from_dev(self, d_planes, plane_stride, plane_pitch, dst, kernel, bias):
        dst, ds = _plane(dst, np.uint8, "dst", True)
        k = _wt(kernel, 800, "kernel")
        h, w = dst.shape
        self._check(self._lib.srcnn_conv55_from_dev(self._h, d_planes, plane_stride, plane_pitch, dst.ctypes.data_as(_u8p), ds,
                                                    w, h, _fp(k), float(bias)))

    def forward_y(self, src, dst=None, preclamp=None):
        """Fused Convolution99x11 + Convolution55 (needs set_weights)."""
        src, ss = _plane(src, np.uint8, "src")
        h, w = src.shape
        if dst is None:
            dst = np.empty((h, w), np.uint8)
        dst, ds = _plane(dst, np.uint8, "dst", True)
        _same_shape("dst", dst.shape, src.shape)
        pp, ps = None, 0
        if preclamp is not None:
            preclamp, ps = _plane(preclamp, np.float32, "preclamp", True)
            _same_shape("preclamp", preclamp.shape, src.shape)
            pp = _fp(preclamp)
        self._check(self._lib.srcnn_forward_y(self._h, src.ctypes.data_as(_u8p), ss,
                                              dst.ctypes.data_as(_u8p), ds, w, h, pp, ps))
        return dst

    def forward_y_frames(self, frames, out=None):
        """A stream of equally sized host frames ([n,h,w] uint8), PCIe transfers overlapped with compute."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 3 or 0 in frames.shape:
            raise ValueError("frames: expected a non-empty [n, h, w] uint8 array")
        n, h, w = frames.shape
        if out is None:
            out = np.empty_like(frames)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8:
            raise TypeError("out: expected a uint8 numpy array")
        _same_shape("out", out.shape, frames.shape)
        if not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out: must be C-contiguous and writeable")
        srcs = (_u8p * n)(*[frames[k].ctypes.data_as(_u8p) for k in range(n)])
        dsts = (_u8p * n)(*[out[k].ctypes.data_as(_u8p) for k in range(n)])
        self._check(self._lib.srcnn_forward_y_frames(self._h, srcs, w, dsts, w, w, h, n))
        return out

    # -- device-resident entry points (integer device addresses) -------------
    def forward_y_dev(self, d_src, src_stride, src_frame_pitch, d_dst, dst_stride, dst_frame_pitch,
                      width, height, n_frames=1, d_preclamp=0):
        self._check(self._lib.srcnn_forward_y_dev(self._h, d_src, src_stride, src_frame_pitch, d_dst,
                                                  dst_stride, dst_frame_pitch, width, height, n_frames,
                                                  d_preclamp or None))

    def forward_y_rows_dev(self, d_src, src_stride, src_row0, d_dst, dst_stride, dst_row0,
                           width, height, row_begin, row_end):
        self._check(self._lib.srcnn_forward_y_rows_dev(self._h, d_src, src_stride, src_row0, d_dst,
                                                       dst_stride, dst_row0, width, height,
                                                       row_begin, row_end))

    def forward_y_rows_halo_dev(self, d_src, src_stride, src_row0, src_rows, d_halo_top, d_halo_bot, halo_stride,
                                d_dst, dst_stride, dst_row0, width, height, row_begin, row_end):
        """A row stripe with its 6 halo rows either side in buffers of their own (0 / None = no rows on that side)."""
        self._check(self._lib.srcnn_forward_y_rows_halo_dev(self._h, d_src, src_stride, src_row0, src_rows,
                                                            d_halo_top or None, d_halo_bot or None, halo_stride, d_dst,
                                                            dst_stride, dst_row0, width, height, row_begin, row_end))

    def halo_transport(self) -> int:
        """0 none yet, 1 same device, 2 peer access (xGMI), 3 staged through the host (srcnn_halo_transport)."""
        return int(self._lib.srcnn_halo_transport(self._h))

    # -- row stripes of every 1-channel model (9-3-5, 9-5-5, zero padding, MODE_BANDED16; 9-1-5 on the strip path) -----------
    def model_halo_rows(self) -> int:
        """Halo rows of the loaded model's stripes: 6 + (f2 - 1) / 2 (srcnn_model_halo_rows)."""
        return int(self._lib.srcnn_model_halo_rows(self._h))

    def model_rows_dev(self, d_src, src_stride, src_row0, d_dst, dst_stride, dst_row0, width, height, row_begin, row_end,
                       d_preclamp=0):
        """Output rows [row_begin, row_end) of a width x height image with whatever forward_y_dev would run for the loaded
        model; d_src starts at image row src_row0 and holds the rows within model_halo_rows() of the range."""
        _stripe_args(width, height, row_begin, row_end, src_stride, dst_stride, src_row0, dst_row0)
        self._check(self._lib.srcnn_model_rows_dev(self._h, d_src, src_stride, src_row0, d_dst, dst_stride, dst_row0, width,
                                                   height, row_begin, row_end, d_preclamp or None))

    def model_rows_halo_dev(self, d_src, src_stride, src_row0, src_rows, d_halo_top, d_halo_bot, halo_stride,
                            d_dst, dst_stride, dst_row0, width, height, row_begin, row_end, d_preclamp=0):
        """The same stripe with its model_halo_rows() halo rows either side in buffers of their own (0 / None = no rows on
        that side); the pointers may point into a neighbour's stripe."""
        _stripe_args(width, height, row_begin, row_end, src_stride, dst_stride, src_row0, dst_row0)
        if src_rows <= 0 or src_row0 + src_rows > height:
            raise ValueError(f"src rows [{src_row0}, {src_row0 + src_rows}) are not rows of a {height}-row image")
        if (d_halo_top or d_halo_bot) and halo_stride < width:
            raise ValueError(f"halo_stride {halo_stride} is less than the width {width}")
        self._check(self._lib.srcnn_model_rows_halo_dev(self._h, d_src, src_stride, src_row0, src_rows, d_halo_top or None,
                                                        d_halo_bot or None, halo_stride, d_dst, dst_stride, dst_row0, width,
                                                        height, row_begin, row_end, d_preclamp or None))

    # -- row stripes of a colour model (packed 3-byte pixels, strides in bytes) and of float planes (strides in floats) --------
    def model_color_rows_dev(self, d_src, src_stride, src_row0, d_dst, dst_stride, dst_row0, width, height, row_begin, row_end,
                             d_preclamp=0):
        """Output rows [row_begin, row_end) of a width x height image of packed 3-byte pixels with what forward_color_dev runs
        for the loaded colour model; d_src starts at image row src_row0 and holds the rows within model_halo_rows() of the
        range.  Strides in bytes (>= 3 * width)."""
        _stripe_args(width, height, row_begin, row_end, src_stride, dst_stride, src_row0, dst_row0, row=3 * width)
        self._check(self._lib.srcnn_model_color_rows_dev(self._h, d_src, src_stride, src_row0, d_dst, dst_stride, dst_row0, width,
                                                         height, row_begin, row_end, d_preclamp or None))

    def model_color_rows_halo_dev(self, d_src, src_stride, src_row0, src_rows, d_halo_top, d_halo_bot, halo_stride,
                                  d_dst, dst_stride, dst_row0, width, height, row_begin, row_end, d_preclamp=0):
        """The same stripe with its model_halo_rows() halo rows either side in buffers of their own (0 / None = no rows on
        that side); the pointers may point into a neighbour's stripe."""
        _stripe_args(width, height, row_begin, row_end, src_stride, dst_stride, src_row0, dst_row0, row=3 * width)
        _halo_args(height, src_row0, src_rows, d_halo_top, d_halo_bot, halo_stride, 3 * width)
        self._check(self._lib.srcnn_model_color_rows_halo_dev(self._h, d_src, src_stride, src_row0, src_rows, d_halo_top or None,
                                                              d_halo_bot or None, halo_stride, d_dst, dst_stride, dst_row0, width,
                                                              height, row_begin, row_end, d_preclamp or None))

    def model_rows_f32_dev(self, d_src, src_stride, src_ch_pitch, src_row0, d_dst, dst_stride, dst_ch_pitch, dst_row0,
                           width, height, row_begin, row_end):
        """Output rows [row_begin, row_end) of a width x height image of float32 planes (1 or 3 by the loaded model) with what
        forward_f32_dev runs; strides and channel pitches in floats, the pitches ignored for one channel."""
        _stripe_args(width, height, row_begin, row_end, src_stride, dst_stride, src_row0, dst_row0)
        _pitch_args(src_ch_pitch, dst_ch_pitch)
        self._check(self._lib.srcnn_model_rows_f32_dev(self._h, d_src, src_stride, src_ch_pitch, src_row0, d_dst, dst_stride,
                                                       dst_ch_pitch, dst_row0, width, height, row_begin, row_end))

    def model_rows_halo_f32_dev(self, d_src, src_stride, src_ch_pitch, src_row0, src_rows, d_halo_top, d_halo_bot, halo_stride,
                                halo_ch_pitch, d_dst, dst_stride, dst_ch_pitch, dst_row0, width, height, row_begin, row_end):
        """The same stripe with its halo rows in buffers of their own, which have a row stride and a channel pitch of their own
        (0 / None = no rows on that side); the pointers may point into a neighbour's stripe."""
        _stripe_args(width, height, row_begin, row_end, src_stride, dst_stride, src_row0, dst_row0)
        _halo_args(height, src_row0, src_rows, d_halo_top, d_halo_bot, halo_stride, width)
        _pitch_args(src_ch_pitch, dst_ch_pitch, halo_ch_pitch)
        self._check(self._lib.srcnn_model_rows_halo_f32_dev(self._h, d_src, src_stride, src_ch_pitch, src_row0, src_rows,
                                                            d_halo_top or None, d_halo_bot or None, halo_stride, halo_ch_pitch,
                                                            d_dst, dst_stride, dst_ch_pitch, dst_row0, width, height, row_begin,
                                                            row_end))

    def forward_y_unfused_dev(self, d_src, src_stride, src_frame_pitch, d_dst, dst_stride,
                              dst_frame_pitch, width, height, n_frames, d_work):
        self._check(self._lib.srcnn_forward_y_unfused_dev(self._h, d_src, src_stride, src_frame_pitch,
                                                          d_dst, dst_stride, dst_frame_pitch, width,
                                                          height, n_frames, d_work))

    def conv99x11_dev(self, d_src, src_stride, d_planes, plane_stride, plane_pitch, width, height):
        self._check(self._lib.srcnn_conv99x11_dev(self._h, d_src, src_stride, d_planes, plane_stride,
                                                  plane_pitch, width, height))

    def conv55_dev(self, d_planes, plane_stride, plane_pitch, d_dst, dst_stride, width, height,
                   d_preclamp=0):
        self._check(self._lib.srcnn_conv55_dev(self._h, d_planes, plane_stride, plane_pitch, d_dst,
                                               dst_stride, width, height, d_preclamp or None))


def scaled_size(width: int, height: int, scale: float):
    """(int)(w*scale), (int)(h*scale) -- src/srcnn.cpp:573-575."""
    ow, oh = C.c_int(), C.c_int()
    rc = load_library().srcnn_scaled_size(width, height, float(scale), C.byref(ow), C.byref(oh))
    if rc != 0:
        raise SrcnnError(rc, "scale too small")
    return ow.value, oh.value


def _image(a, name, writable=False):
    if not isinstance(a, np.ndarray) or a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise TypeError(f"{name}: expected an HxWx3 uint8 array (B,G,R)")
    if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        raise ValueError(f"{name}: pixels must be packed B,G,R (row stride may be padded)")
    if writable and not a.flags.writeable:
        raise ValueError(f"{name}: output image is read-only")
    return a, a.strides[0]


def _ctx_method(fn):
    setattr(Context, fn.__name__, fn)
    return fn


@_ctx_method
def bgr2ycrcb(self, bgr):
    """cvtColor(CV_BGR2YCrCb) + split (src/srcnn.cpp:509,540) -> (y, cr, cb) planes."""
    bgr, st = _image(bgr, "bgr")
    h, w, _ = bgr.shape
    out = [np.empty((h, w), np.uint8) for _ in range(3)]
    self._check(self._lib.srcnn_bgr2ycrcb(self._h, bgr.ctypes.data_as(_u8p), st, w, h,
                                          *[o.ctypes.data_as(_u8p) for o in out], w))
    return out


@_ctx_method
def ycrcb2bgr(self, y, cr, cb):
    """merge + cvtColor(CV_YCrCb2BGR) (src/srcnn.cpp:639,657) -> HxWx3 B,G,R."""
    planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in (y, cr, cb)]
    h, w = planes[0].shape
    out = np.empty((h, w, 3), np.uint8)
    self._check(self._lib.srcnn_ycrcb2bgr(self._h, *[p.ctypes.data_as(_u8p) for p in planes], w, w, h,
                                          out.ctypes.data_as(_u8p), 3 * w))
    return out


@_ctx_method
def resize_cubic(self, src, dst_w, dst_h):
    """resize(.., CV_INTER_CUBIC) of one 8-bit plane (src/srcnn.cpp:577-582)."""
    src, ss = _plane(src, np.uint8, "src")
    h, w = src.shape
    out = np.empty((dst_h, dst_w), np.uint8)
    self._check(self._lib.srcnn_resize_cubic(self._h, src.ctypes.data_as(_u8p), ss, w, h,
                                             out.ctypes.data_as(_u8p), dst_w, dst_w, dst_h))
    return out


@_ctx_method
def process_bgr(self, bgr, scale):
    """The reference's timed pipeline region (src/srcnn.cpp:505-659) in one call."""
    bgr, st = _image(bgr, "bgr")
    h, w, _ = bgr.shape
    ow, oh = scaled_size(w, h, scale)
    out = np.empty((oh, ow, 3), np.uint8)
    self._check(self._lib.srcnn_process_bgr(self._h, bgr.ctypes.data_as(_u8p), st, w, h, float(scale),
                                            out.ctypes.data_as(_u8p), 3 * ow))
    return out


@_ctx_method
def process_bgr_dev(self, d_bgr, stride, width, height, scale, d_out, out_stride):
    self._check(self._lib.srcnn_process_bgr_dev(self._h, d_bgr, stride, width, height, float(scale),
                                                d_out, out_stride))


def cubic_f32_taps(src_n: int, dst_n: int):
    """The float resize's table of one axis (srcnn_cubic_f32_taps; host only, needs no GPU): (first, coef) with first[d] the
    unclamped floor of the source coordinate of output d (int32, taps first - 1 .. first + 2) and coef[d] its four float32
    coefficients."""
    if src_n <= 0 or dst_n <= 0:
        raise ValueError(f"cubic_f32_taps: sizes {src_n} -> {dst_n} (both must be positive)")
    first = np.empty(dst_n, np.int32)
    coef = np.empty((dst_n, 4), np.float32)
    rc = load_library().srcnn_cubic_f32_taps(int(src_n), int(dst_n), first.ctypes.data_as(C.POINTER(C.c_int)), _fp(coef))
    if rc != 0:
        raise SrcnnError(rc, "cubic_f32_taps")
    return first, coef


class ChromaGrid:
    """Where a frame's chroma samples lie: sub_x, sub_y luma samples per chroma sample (1 or 2 each), and chroma
    sample j at j + 0.5 + d in chroma samples -- d = 0 centred, -0.25 co-sited with the even luma sample, +0.25 with the odd
    one; |d| <= 0.5, and 0 on an axis that is not subsampled.  ValueError otherwise."""
    __slots__ = ("sub_x", "sub_y", "dx", "dy")

    def __init__(self, sub_x=2, sub_y=2, dx=0.0, dy=0.0):
        for name, sub, d in (("x", sub_x, dx), ("y", sub_y, dy)):
            if isinstance(sub, bool) or sub not in (1, 2):
                raise ValueError(f"ChromaGrid: sub_{name} {sub!r}: expected 1 or 2")
            try:
                d = float(d)
            except (TypeError, ValueError):
                raise ValueError(f"ChromaGrid: d{name} {d!r}: expected a number") from None
            if not abs(d) <= 0.5:
                raise ValueError(f"ChromaGrid: d{name} {d!r}: expected a finite offset of at most 0.5 chroma samples")
            if sub == 1 and d != 0.0:
                raise ValueError(f"ChromaGrid: d{name} {d!r} on an axis that is not subsampled (sub_{name} = 1): expected 0")
        self.sub_x, self.sub_y, self.dx, self.dy = int(sub_x), int(sub_y), float(dx), float(dy)

    def plane(self, width: int, height: int):
        """(chroma width, chroma height) of a frame of width x height luma samples."""
        return -(-int(width) // self.sub_x), -(-int(height) // self.sub_y)

    def __eq__(self, other):
        return isinstance(other, ChromaGrid) and (self.sub_x, self.sub_y, self.dx, self.dy) == (other.sub_x, other.sub_y, other.dx, other.dy)

    def __repr__(self):
        return f"ChromaGrid(sub_x={self.sub_x}, sub_y={self.sub_y}, dx={self.dx}, dy={self.dy})"


_SUBSAMPLING = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
# ffmpeg's chroma_sample_location names -> (dx, dy) in chroma samples on a subsampled axis
_CHROMA_LOC = {"left": (-0.25, 0.0), "center": (0.0, 0.0), "topleft": (-0.25, -0.25), "top": (0.0, -0.25),
               "bottomleft": (-0.25, 0.25), "bottom": (0.0, 0.25)}


def chroma_grid(subsampling: str = "420", chroma_loc: str = "left") -> ChromaGrid:
    """The ChromaGrid of a pixel format and ffmpeg's chroma_sample_location: subsampling "420", "422" or "444"; chroma_loc
    "left" (H.264, HEVC, MPEG-2), "center" (JPEG, MPEG-1), "topleft" (BT.2020), "top", "bottomleft" or "bottom".  -0.25, 0 or
    +0.25 per axis, and 0 on an axis that is not subsampled."""
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: expected '420', '422' or '444'")
    if chroma_loc not in _CHROMA_LOC:
        raise ValueError(f"chroma_loc {chroma_loc!r}: expected one of {', '.join(map(repr, _CHROMA_LOC))}")
    (sx, sy), (dx, dy) = _SUBSAMPLING[subsampling], _CHROMA_LOC[chroma_loc]
    return ChromaGrid(sx, sy, dx if sx == 2 else 0.0, dy if sy == 2 else 0.0)


def chroma_taps(src_len: int, dst_len: int, src_sub: int = 2, dst_sub: int = 2, src_d: float = 0.0, dst_d: float = 0.0):
    """The sited table of one axis (srcnn_chroma_taps; host only, needs no GPU): (first, coef) for the ceil(dst_len / dst_sub)
    chroma samples of an axis of dst_len LUMA samples, read from the chroma samples of an axis of src_len luma samples."""
    import math
    if src_len <= 0 or dst_len <= 0:
        raise ValueError(f"chroma_taps: luma lengths {src_len} -> {dst_len} (both must be positive)")
    for sub, d in ((src_sub, src_d), (dst_sub, dst_d)):
        if sub not in (1, 2) or not math.isfinite(d) or abs(d) > 0.5 or (sub == 1 and d != 0):
            raise ValueError(f"chroma_taps: sub {sub!r}, d {d!r}: expected a sub of 1 or 2 and |d| <= 0.5, 0 where the sub is 1")
    n = -(-int(dst_len) // int(dst_sub))
    first = np.empty(n, np.int32)
    coef = np.empty((n, 4), np.float32)
    rc = load_library().srcnn_chroma_taps(int(src_len), int(dst_len), int(src_sub), int(dst_sub), float(src_d), float(dst_d),
                                          first.ctypes.data_as(C.POINTER(C.c_int)), _fp(coef))
    if rc != 0:
        raise SrcnnError(rc, "chroma_taps")
    return first, coef


def cubic_aa_f32_taps(src_n: int, dst_n: int):
    """The antialiased resize's table of one axis (srcnn_cubic_aa_f32_taps; host only, needs no GPU): (first, count, coef) with
    first[d] the first source sample of output d, count[d] its tap count (int32 both) and coef[d, :count[d]] its float32
    coefficients, zero beyond; coef has as many columns as the largest count."""
    if src_n <= 0 or dst_n <= 0:
        raise ValueError(f"cubic_aa_f32_taps: sizes {src_n} -> {dst_n} (both must be positive)")
    lib = load_library()
    k = lib.srcnn_cubic_aa_f32_taps(int(src_n), int(dst_n), None, None, None, 0)
    if k <= 0:
        raise SrcnnError(k, "cubic_aa_f32_taps")
    first, count = np.empty(dst_n, np.int32), np.empty(dst_n, np.int32)
    coef = np.empty((dst_n, k), np.float32)
    ip = C.POINTER(C.c_int)
    rc = lib.srcnn_cubic_aa_f32_taps(int(src_n), int(dst_n), first.ctypes.data_as(ip), count.ctypes.data_as(ip), _fp(coef), k)
    if rc != k:
        raise SrcnnError(rc, "cubic_aa_f32_taps")
    return first, count, coef


def pil_taps(src_n: int, dst_n: int, filter: int = PIL_BICUBIC):
    """Pillow's table of one axis for uint8 pictures (srcnn_pil_taps; host only, needs no GPU): (first, count, coef) with
    first[d] the first source sample of output d, count[d] its tap count and coef[d, :count[d]] its int32 coefficients with 22
    fractional bits, zero beyond; coef has as many columns as the largest count.  filter: PIL_BILINEAR or PIL_BICUBIC."""
    if src_n <= 0 or dst_n <= 0:
        raise ValueError(f"pil_taps: sizes {src_n} -> {dst_n} (both must be positive)")
    if filter not in (PIL_BILINEAR, PIL_BICUBIC):
        raise ValueError(f"pil_taps: filter {filter!r}: expected PIL_BILINEAR (2) or PIL_BICUBIC (3)")
    lib = load_library()
    k = lib.srcnn_pil_taps(int(src_n), int(dst_n), int(filter), None, None, None, 0)
    if k <= 0:
        raise SrcnnError(k, "pil_taps")
    first, count = np.empty(dst_n, np.int32), np.empty(dst_n, np.int32)
    coef = np.empty((dst_n, k), np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.srcnn_pil_taps(int(src_n), int(dst_n), int(filter), first.ctypes.data_as(ip), count.ctypes.data_as(ip),
                            coef.ctypes.data_as(C.POINTER(C.c_int32)), k)
    if rc != k:
        raise SrcnnError(rc, "pil_taps")
    return first, count, coef


def luma_bt601_studio(value_range: float = 1.0):
    """The luma row of BT.601 studio range (MATLAB's rgb2ycbcr) for R, G, B planes holding [0, value_range]:
    (65.481, 128.553, 24.966) / 255 with the offset 16 / 255 * value_range."""
    return (65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0, 16.0 / 255.0 * float(value_range))


def luma_for_order(luma, order: str = "rgb"):
    """A luma row given for R, G, B planes as the row for planes in `order`: "rgb" (unchanged) or "bgr" (the three weights
    reversed, the offset kept)."""
    w0, w1, w2, off = luma
    if order == "rgb":
        return (w0, w1, w2, off)
    if order == "bgr":
        return (w2, w1, w0, off)
    raise ValueError(f"order {order!r}: expected 'rgb' or 'bgr'")


def _luma4(luma):
    """{w0, w1, w2, offset} as a C array of four floats: ValueError unless four finite numbers whose weights (as float32) sum to
    more than 0, before any call into the library."""
    try:
        a = np.asarray(luma, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"luma {luma!r}: expected four numbers (w0, w1, w2, offset)") from None
    if a.size != 4 or not np.isfinite(a).all() or not float(a[:3].astype(np.float64).sum()) > 0.0:
        raise ValueError(f"luma {luma!r}: expected four finite numbers (w0, w1, w2, offset) with w0 + w1 + w2 > 0")
    return (C.c_float * 4)(*a.tolist())


def _metric_luma4(luma):
    """None, or {w0, w1, w2, offset} of a metric as a C array of four floats: ValueError unless four finite numbers (as float32),
    before any call into the library.  (A metric's luma need not be invertible: the weights may sum to anything.)"""
    if luma is None:
        return None
    try:
        a = np.asarray(luma, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"luma {luma!r}: expected None or four numbers (w0, w1, w2, offset)") from None
    if a.size != 4 or not np.isfinite(a).all():
        raise ValueError(f"luma {luma!r}: expected None or four finite numbers (w0, w1, w2, offset)")
    return (C.c_float * 4)(*a.tolist())


def metric_psnr(sse: float, n_px: float, data_range: float = 1.0) -> float:
    """10 log10(L^2 n_px / sse) from the sums metrics_image_dev returns (srcnn_metric_psnr; host only, needs no GPU): inf for
    sse == 0, nan for arguments that are no sums."""
    return float(load_library().srcnn_metric_psnr(float(sse), float(n_px), float(data_range)))


def metric_msssim(sums, weights=None) -> float:
    """MS-SSIM from the (n_scales, 3) sums msssim_image_dev returns for one result (srcnn_metric_msssim; host only, needs no
    GPU): the product over the scales of max(mean, 0)^w, the mean of cs below the last scale and of ssim at it.  weights=None:
    MSSSIM_WEIGHTS, which needs five scales.  nan for arguments that are no sums; 0 where a mean is not positive."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != 3:
        raise ValueError(f"sums of shape {s.shape}: expected (n_scales, 3) rows of (cs_sum, ssim_sum, n_win)")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != s.shape[0]:
            raise ValueError(f"{w.size} weights for {s.shape[0]} scales")
    dp = C.POINTER(C.c_double)
    return float(load_library().srcnn_metric_msssim(s.ctypes.data_as(dp), int(s.shape[0]), None if w is None else w.ctypes.data_as(dp)))


def _clamp2(clamp):
    """None, or (lo, hi) as a C array of two floats: ValueError unless lo <= hi and neither is a NaN."""
    if clamp is None:
        return None
    try:
        lo, hi = (float(np.float32(v)) for v in clamp)
    except (TypeError, ValueError):
        raise ValueError(f"clamp {clamp!r}: expected None or (lo, hi)") from None
    if not lo <= hi:
        raise ValueError(f"clamp {clamp!r}: expected lo <= hi, neither a NaN")
    return (C.c_float * 2)(lo, hi)


def _not_shrinking(w, h, dst_w, dst_h):
    if dst_w < w or dst_h < h:
        raise ValueError(f"{h} x {w} -> {dst_h} x {dst_w} (H x W) shrinks the image: a super-resolution call resizes up or not at all")


class Image:
    """Where an image lies and what its elements are (srcnn_image): element (f, c, y, x) at ptr + f * frame_pitch + c * ch_pitch
    + y * stride + x * px_step, all in elements of `elem` (ELEM_*).  Planar NCHW: px_step 1; channels-last or H x W x C: px_step
    C, ch_pitch 1; RGBA with the alpha skipped: px_step 4, ch_pitch 1, three channels.  scale: ELEM_U8 only -- a load is byte *
    scale, a store rint(clamp(value * scale, 0, 255)).  A pitch whose count is 1 is ignored.
    An Image is an address and steps: it keeps no tensor or buffer alive.  Whoever builds one holds the memory for as long as a
    call that was given the Image may run (a freed block of a caching allocator still seems to work, until it is unmapped)."""
    __slots__ = ("ptr", "elem", "px_step", "stride", "ch_pitch", "frame_pitch", "scale")

    def __init__(self, ptr, elem=ELEM_F32, px_step=1, stride=0, ch_pitch=0, frame_pitch=0, scale=1.0):
        self.ptr, self.elem, self.px_step, self.stride = int(ptr), int(elem), int(px_step), int(stride)
        self.ch_pitch, self.frame_pitch, self.scale = int(ch_pitch), int(frame_pitch), float(scale)

    def c(self) -> _CImage:
        for v in (self.px_step, self.stride, self.ch_pitch, self.frame_pitch):
            if v < 0:
                raise ValueError(f"{self!r}: steps and pitches must not be negative")
        return _CImage(self.ptr, self.elem, self.scale, self.px_step, self.stride, self.ch_pitch, self.frame_pitch)

    def __repr__(self):
        return (f"Image(ptr={self.ptr:#x}, elem={self.elem}, px_step={self.px_step}, stride={self.stride}, ch_pitch={self.ch_pitch}, "
                f"frame_pitch={self.frame_pitch}, scale={self.scale})")


def image_check(image: Image, width: int, height: int, channels: int, n_frames: int = 1, is_dst: bool = False) -> bool:
    """srcnn_image_check (host only, needs no GPU): whether the library accepts the descriptor for an image of that size -- as a
    destination only where its address map is shown injective (every step, sorted, exceeds what the smaller ones reach)."""
    return load_library().srcnn_image_check(C.byref(image.c()), int(width), int(height), int(channels), int(n_frames),
                                            int(bool(is_dst))) == 0


def luma_gain(luma) -> float:
    """g = 1 / (w0 + w1 + w2) of a luma row as process_rgb_f32 uses it (srcnn_luma_gain; host only, needs no GPU): the sum in
    float64 over the float32 weights, rounded once to float32."""
    g = C.c_float()
    rc = load_library().srcnn_luma_gain(_luma4(luma), C.byref(g))
    if rc != 0:
        raise SrcnnError(rc, "luma_gain")
    return float(g.value)


def stripe_rows(height: int, n_parts: int, index: int):
    """[begin, end) of part `index` of `n_parts` (srcnn_stripe_rows; equals sharding.split_range)."""
    a, b = C.c_int(), C.c_int()
    rc = load_library().srcnn_stripe_rows(height, n_parts, index, C.byref(a), C.byref(b))
    if rc != 0:
        raise SrcnnError(rc, "bad split")
    return a.value, b.value


def _ctx_array(ctxs):
    if not ctxs:
        raise ValueError("need at least one context")
    return (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])


def forward_y_frames_multi(ctxs: Sequence[Context], frames, out=None):
    """A stream of host frames over several contexts / GPUs (srcnn_forward_y_frames_multi)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    if frames.ndim != 3 or 0 in frames.shape:
        raise ValueError("frames: expected a non-empty [n, h, w] uint8 array")
    n, h, w = frames.shape
    if out is None:
        out = np.empty_like(frames)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8:
        raise TypeError("out: expected a uint8 numpy array")
    _same_shape("out", out.shape, frames.shape)
    if not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError("out: must be C-contiguous and writeable")
    srcs = (_u8p * n)(*[frames[k].ctypes.data_as(_u8p) for k in range(n)])
    dsts = (_u8p * n)(*[out[k].ctypes.data_as(_u8p) for k in range(n)])
    ctxs[0]._check_multi(ctxs, load_library().srcnn_forward_y_frames_multi(_ctx_array(ctxs), len(ctxs), srcs, w, dsts, w,
                                                                          w, h, n))
    return out


def forward_y_lanes_dev(ctxs: Sequence[Context], d_src_ptrs, src_stride, d_dst_ptrs, dst_stride, width, height):
    """Device-resident planes of a stream over the contexts used as lanes: plane f on ctxs[f % len(ctxs)], asynchronous
    (srcnn_forward_y_lanes_dev).  Two contexts on one GPU = two lanes of it."""
    n = len(d_src_ptrs)
    if n == 0 or len(d_dst_ptrs) != n:
        raise ValueError("need as many output planes as input planes, at least one")
    srcs = (C.c_void_p * n)(*[int(p) for p in d_src_ptrs])
    dsts = (C.c_void_p * n)(*[int(p) for p in d_dst_ptrs])
    ctxs[0]._check_multi(ctxs, load_library().srcnn_forward_y_lanes_dev(_ctx_array(ctxs), len(ctxs), srcs, src_stride, dsts, dst_stride,
                                                                       width, height, n))


def forward_y_striped(ctxs: Sequence[Context], src, dst=None):
    """ONE host plane row-striped over several contexts / GPUs (srcnn_forward_y_striped)."""
    src, ss = _plane(src, np.uint8, "src")
    h, w = src.shape
    if dst is None:
        dst = np.empty((h, w), np.uint8)
    dst, ds = _plane(dst, np.uint8, "dst", True)
    _same_shape("dst", dst.shape, src.shape)
    ctxs[0]._check_multi(ctxs, load_library().srcnn_forward_y_striped(_ctx_array(ctxs), len(ctxs), src.ctypes.data_as(_u8p),
                                                                     ss, dst.ctypes.data_as(_u8p), ds, w, h))
    return dst


def forward_y_striped_frames(ctxs: Sequence[Context], planes, out=None):
    """A STREAM of host planes [n, h, w], each row-striped over the contexts, pipelined (srcnn_forward_y_striped_frames)."""
    if not isinstance(planes, np.ndarray) or planes.dtype != np.uint8 or planes.ndim != 3 or not planes.flags.c_contiguous:
        raise ValueError("planes: expected a C-contiguous [n, h, w] uint8 array")
    n, h, w = planes.shape
    if out is None:
        out = np.empty_like(planes)
    _same_shape("out", out.shape, planes.shape)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError("out: must be a C-contiguous writeable uint8 array")
    srcs = (_u8p * n)(*[planes[k].ctypes.data_as(_u8p) for k in range(n)])
    dsts = (_u8p * n)(*[out[k].ctypes.data_as(_u8p) for k in range(n)])
    ctxs[0]._check_multi(ctxs, load_library().srcnn_forward_y_striped_frames(_ctx_array(ctxs), len(ctxs), srcs, w, dsts, w, w, h, n))
    return out


def forward_y_striped_dev(ctxs: Sequence[Context], d_stripes, stripe_stride, d_out, out_stride, width, height):
    """Device-resident striped step: d_stripes[k] / d_out[k] are integer device addresses on ctxs[k]'s GPU."""
    n = len(ctxs)
    ins = (C.c_void_p * n)(*[int(p) for p in d_stripes])
    outs = (C.c_void_p * n)(*[int(p) for p in d_out])
    ctxs[0]._check_multi(ctxs, load_library().srcnn_forward_y_striped_dev(_ctx_array(ctxs), n, ins, stripe_stride, outs,
                                                                         out_stride, width, height))


def _stripe_args(width, height, row_begin, row_end, src_stride, dst_stride, src_row0, dst_row0, row=None):
    """The geometry of a stripe call, checked before the library is entered.  row: elements of a row (3 * width for packed
    3-byte pixels), the width by default."""
    if width <= 0 or height <= 0:
        raise ValueError(f"empty image {width} x {height}")
    if not 0 <= row_begin < row_end <= height:
        raise ValueError(f"rows [{row_begin}, {row_end}) are not a row range of a {height}-row image")
    row = width if row is None else row
    if src_stride < row or dst_stride < row:
        raise ValueError(f"row strides {src_stride} / {dst_stride} are less than the row of {row} elements")
    if not 0 <= src_row0 <= row_begin or not 0 <= dst_row0 <= row_begin:
        raise ValueError(f"src_row0 {src_row0} / dst_row0 {dst_row0} must lie in [0, row_begin = {row_begin}]")


def _halo_args(height, src_row0, src_rows, d_halo_top, d_halo_bot, halo_stride, row):
    if src_rows <= 0 or src_row0 + src_rows > height:
        raise ValueError(f"src rows [{src_row0}, {src_row0 + src_rows}) are not rows of a {height}-row image")
    if (d_halo_top or d_halo_bot) and halo_stride < row:
        raise ValueError(f"halo_stride {halo_stride} is less than the row of {row} elements")


def _pitch_args(*pitches):
    if any(p < 0 for p in pitches):
        raise ValueError(f"channel pitches {pitches} must not be negative")


def _striped_dev_args(ctxs, d_stripes, stripe_stride, d_out, out_stride, width, height, row):
    handles, n = _ctx_array(ctxs), len(ctxs)
    if len(d_stripes) != n or len(d_out) != n:
        raise ValueError(f"need one input and one output stripe per context: {len(d_stripes)} / {len(d_out)} for {n} contexts")
    if width <= 0 or height <= 0 or stripe_stride < row or out_stride < row:
        raise ValueError(f"bad geometry: {width} x {height}, strides {stripe_stride} / {out_stride} for rows of {row} elements")
    return handles, n, (C.c_void_p * n)(*[int(p) for p in d_stripes]), (C.c_void_p * n)(*[int(p) for p in d_out])


def model_color_striped(ctxs: Sequence[Context], img, dst=None):
    """ONE host image (H, W, 3) of packed 3-byte pixels row-striped over several contexts / GPUs that hold the same colour model
    (srcnn_model_color_striped); bit-identical to forward_color."""
    handles = _ctx_array(ctxs)
    img, ss = _image(img, "img")
    h, w, _ = img.shape
    if dst is None:
        dst = np.empty((h, w, 3), np.uint8)
    dst, ds = _image(dst, "dst", True)
    _same_shape("dst", dst.shape, img.shape)
    ctxs[0]._check_multi(ctxs, load_library().srcnn_model_color_striped(handles, len(ctxs), img.ctypes.data_as(_u8p), ss,
                                                                       dst.ctypes.data_as(_u8p), ds, w, h))
    return dst


def model_color_striped_dev(ctxs: Sequence[Context], d_stripes, stripe_stride, d_out, out_stride, width, height):
    """Device-resident striped step of the same: d_stripes[k] / d_out[k] are integer device addresses on ctxs[k]'s GPU of that
    context's rows stripe_rows(height, len(ctxs), k), strides in bytes (>= 3 * width).  Asynchronous; the caller orders it."""
    handles, n, ins, outs = _striped_dev_args(ctxs, d_stripes, stripe_stride, d_out, out_stride, width, height, 3 * width)
    ctxs[0]._check_multi(ctxs, load_library().srcnn_model_color_striped_dev(handles, n, ins, stripe_stride, outs, out_stride,
                                                                           width, height))


def model_striped_f32(ctxs: Sequence[Context], x, out=None):
    """ONE host image of float32 planes, (H, W) or (C, H, W) with any row / channel stride, row-striped over several contexts /
    GPUs that hold the same model (srcnn_model_striped_f32); bit-identical to forward_f32."""
    handles = _ctx_array(ctxs)
    if isinstance(x, np.ndarray) and x.ndim == 4:
        raise TypeError("x: expected one image, (H, W) or (C, H, W)")
    x4 = _f32_planes(x, "x")
    if out is None:
        out = np.empty(x.shape, np.float32)
    o4 = _f32_planes(out, "out", True)
    _same_shape("out", out.shape, x.shape)
    _, c, h, w = x4.shape
    if c not in (1, 3):
        raise ValueError(f"x: shape {tuple(x.shape)}: a model has 1 channel or 3")
    stride = lambda a4: a4.strides[2] // 4 if h > 1 else w
    ctxs[0]._check_multi(ctxs, load_library().srcnn_model_striped_f32(handles, len(ctxs), _fp(x4[0]), stride(x4),
                                                                     x4.strides[1] // 4 if c > 1 else 0, _fp(o4[0]), stride(o4),
                                                                     o4.strides[1] // 4 if c > 1 else 0, w, h))
    return out


def model_striped_f32_dev(ctxs: Sequence[Context], d_stripes, stripe_stride, stripe_ch_pitch, d_out, out_stride, out_ch_pitch,
                          width, height):
    """Device-resident striped step of the same: strides and channel pitches in floats, one stride and one pitch for all the
    stripes (and all the outputs).  Asynchronous; the caller orders it."""
    handles, n, ins, outs = _striped_dev_args(ctxs, d_stripes, stripe_stride, d_out, out_stride, width, height, width)
    _pitch_args(stripe_ch_pitch, out_ch_pitch)
    ctxs[0]._check_multi(ctxs, load_library().srcnn_model_striped_f32_dev(handles, n, ins, stripe_stride, stripe_ch_pitch, outs,
                                                                         out_stride, out_ch_pitch, width, height))


def model_striped(ctxs: Sequence[Context], src, dst=None):
    """ONE host plane row-striped over several contexts / GPUs with whatever forward_y would run for the model they hold
    (srcnn_model_striped): 9-3-5, 9-5-5, zero padding, MODE_BANDED16; a 9-1-5 model on the strip path runs forward_y_striped."""
    handles = _ctx_array(ctxs)
    src, ss = _plane(src, np.uint8, "src")
    h, w = src.shape
    if dst is None:
        dst = np.empty((h, w), np.uint8)
    dst, ds = _plane(dst, np.uint8, "dst", True)
    _same_shape("dst", dst.shape, src.shape)
    ctxs[0]._check_multi(ctxs, load_library().srcnn_model_striped(handles, len(ctxs), src.ctypes.data_as(_u8p), ss,
                                                                 dst.ctypes.data_as(_u8p), ds, w, h))
    return dst


def model_striped_dev(ctxs: Sequence[Context], d_stripes, stripe_stride, d_out, out_stride, width, height):
    """Device-resident striped step of the same: d_stripes[k] / d_out[k] are integer device addresses on ctxs[k]'s GPU of that
    context's rows stripe_rows(height, len(ctxs), k).  Asynchronous; the caller orders it behind whatever wrote the stripes."""
    handles, n = _ctx_array(ctxs), len(ctxs)
    if len(d_stripes) != n or len(d_out) != n:
        raise ValueError(f"need one input and one output stripe per context: {len(d_stripes)} / {len(d_out)} for {n} contexts")
    if width <= 0 or height <= 0 or stripe_stride < width or out_stride < width:
        raise ValueError(f"bad geometry: {width} x {height}, strides {stripe_stride} / {out_stride}")
    ins = (C.c_void_p * n)(*[int(p) for p in d_stripes])
    outs = (C.c_void_p * n)(*[int(p) for p in d_out])
    ctxs[0]._check_multi(ctxs, load_library().srcnn_model_striped_dev(handles, n, ins, stripe_stride, outs, out_stride,
                                                                     width, height))


def _check_multi(self, ctxs, rc):
    if rc != 0:
        msgs = [self._lib.srcnn_last_error(c._h).decode() for c in ctxs]
        raise SrcnnError(rc, " | ".join(m for m in msgs if m != "no error") or "multi-context call failed")


Context._check_multi = _check_multi

_default: Optional[Context] = None


def default_context() -> Context:
    global _default
    if _default is None:
        _default = Context(0)
    return _default


# The reference's free functions (src/srcnn.cpp:60-73), same names and argument order.
def Convolution99(src, dst, kernel, bias):
    default_context().conv99(src, dst, kernel, bias)


def Convolution11(src: Sequence[np.ndarray], dst, kernel, bias):
    default_context().conv11(src, dst, kernel, bias)


def Convolution55(src: Sequence[np.ndarray], dst, kernel, bias):
    default_context().conv55(src, dst, kernel, bias)


def Convolution99x11(src, dst: Sequence[np.ndarray], kernel99, bias99, kernel11, bias11):
    default_context().conv99x11(src, dst, kernel99, bias99, kernel11, bias11)
