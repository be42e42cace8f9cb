"""The reference of the image calls' load and store (include/srcnn_amd.h, srcnn_image): numpy conversions between float32 and the
stored element kinds, as BITS (float16 and bfloat16 as uint16, so that numpy needs no bfloat16), and the layouts the GPU tests
use.  Own code; nothing here calls the library under test.  tests/test_image_cpu.py pins these conversions to torch's CPU ops."""
import numpy as np

F32, F16, BF16, U8 = 0, 1, 2, 3                      # SRCNN_ELEM_*
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16, U8: np.uint8}


def load(bits, elem, scale=1.0):
    """Stored bits -> float32: F32 as it is, F16 and BF16 widened exactly, U8 (float)b * scale with one rounding."""
    bits = np.asarray(bits, dtype=BITS[elem])
    if elem == F32:
        return bits.view(np.float32)
    if elem == F16:
        return bits.view(np.float16).astype(np.float32)
    if elem == BF16:
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.astype(np.float32) * np.float32(scale)


def store(v, elem, scale=1.0):
    """float32 -> stored bits.  F16: round to nearest even, overflow to +-inf; BF16: round to nearest even; both keep a NaN a
    NaN; U8: t = v * scale (one rounding), rint_half_even(min(max(t, 0), 255)), 0 for a NaN."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if elem == F32:
        return v.view(np.uint32)
    if elem == F16:
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    if elem == BF16:
        u = v.view(np.uint32)
        rounded = (u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16
        nan = (u & 0x7FFFFFFF) > 0x7F800000
        return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * np.float32(scale)
        t = np.where(t >= 0, t, np.float32(0))          # a NaN fails the comparison: 0
        t = np.where(t > 255, np.float32(255), t)
        return np.rint(t).astype(np.uint8)


def is_nan_bits(bits, elem):
    if elem == F32:
        return (bits & 0x7FFFFFFF) > 0x7F800000
    if elem == F16:
        return (bits & 0x7FFF) > 0x7C00
    if elem == BF16:
        return (bits & 0x7FFF) > 0x7F80
    return np.zeros(bits.shape, bool)


def same_stored(got, want, elem):
    """Bitwise equality of stored arrays; two NaNs are equal whatever their payload."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    g, w = is_nan_bits(got, elem), is_nan_bits(want, elem)
    return bool(np.array_equal(g, w) and np.array_equal(got[~g], want[~w]))


def half_ulp(ref, elem):
    """Half a unit in the last place of the stored format at |ref| (float64 array): the store's own rounding error."""
    a = np.maximum(np.abs(np.asarray(ref, dtype=np.float64)), 2.0 ** (-14 if elem == F16 else -126))
    e = np.floor(np.log2(a))
    return 0.5 * 2.0 ** (e - (10 if elem == F16 else 7))


# ---- layouts: (px_step, stride, ch_pitch, frame_pitch) in elements for a (n, c, h, w) image --------------------------------
def layout(kind, c, h, w, row_pad=0, frame_pad=0):
    """planar: NCHW.  interleaved: H x W x C pixels (one channel: a channel of a 3-channel interleaved image, px_step 3).
    rgba: 4-element pixels of which the first c are the image's."""
    if kind == "planar":
        stride = w + row_pad
        return 1, stride, h * stride, c * h * stride + frame_pad
    px = 4 if kind == "rgba" else (c if c > 1 else 3)
    stride = w * px + row_pad
    return px, stride, 1, h * stride + frame_pad


# (name, element kind, layout kind): the formats of the GPU tests
FORMATS = [("planar-f32", F32, "planar"), ("interleaved-f32", F32, "interleaved"), ("interleaved-f16", F16, "interleaved"),
           ("planar-bf16", BF16, "planar"), ("interleaved-u8", U8, "interleaved"), ("rgba-u8", U8, "rgba")]
