"""A PyTorch SRCNN module on this library's kernels: float32 tensors on the GPU in, float32 tensors out.

    from srcnn_cpp_amd.torch_api import compile_module
    fast = compile_module(module)              # an nn.Module with conv1, conv2, conv3 (9-f2-5, 1 or 3 channels)
    y = fast(x)                                # x: float32 (N, C, H, W) or (C, H, W) on that GPU; y ~ module(x)
    z = fast.upscale(lr, scale=2)              # ~ module(F.interpolate(lr, size, mode="bicubic", align_corners=False))
    lr = fast.resize(hr, (h // 2, w // 2), antialias=True)   # the way down: F.interpolate(..., antialias=True)
    rgb = fast.upscale_rgb(lr_rgb, scale=2)    # a 1-channel module on the luma of an RGB tensor, chroma resized, merged
    out = fast.upscale_rgb_image(torch.from_numpy(hwc_u8).cuda().permute(2, 0, 1), scale=2)   # H x W x 3 uint8 in and out
    db, q = fast.psnr(sr, hr, border=2), fast.ssim(sr, hr, border=2)   # float64 (N, P): the measurement, on stored tensors

The *_image methods (forward_image, resize_image, upscale_image, upscale_rgb_image) take the tensor in the format it is stored
in: float32, float16, bfloat16 or uint8, any positive strides (a permuted H x W x C view, channels_last, padded rows), and write
the dtype and layout asked for.  A uint8 tensor is read as byte * in_scale (1 / 255) and written as
round(clamp(value * out_scale, 0, 255)) (255); between load and store the arithmetic is that of the float32 methods, bit for bit.

The weights go in as they are (the data is already in the model's units), the module's padding mode is the context's padding,
the call runs on torch.cuda.current_stream() and reads the tensor where it lies: data_ptr() and strides, no copy.  torch is
imported when compile_module is called, not when this module is.
"""
from __future__ import annotations

from . import (ELEM_BF16, ELEM_F16, ELEM_F32, ELEM_U8, LUMA_BT601, MODE_BANDED16, MODE_MFMA, Context, Image, _clamp2, _luma4,
               model_from_module)

__all__ = ["compile_module", "CompiledModule"]


def check_input(x, channels: int, device_index: int):
    """ValueError unless x is a float32 CUDA tensor (N, C, H, W) or (C, H, W) on GPU `device_index` with C = channels, rows
    contiguous and the other strides positive.  Returns (n, h, w, row stride, channel pitch, frame pitch) in elements.  Runs
    before any call into the library."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"expected a float32 tensor, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"expected shape (N, {channels}, H, W) or ({channels}, H, W), got {tuple(x.shape)}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    n, c, h, w = x.shape
    if c != channels:
        raise ValueError(f"the module has {channels} channel(s), the tensor {c}: shape {tuple(x.shape)}")
    if 0 in (n, h, w):
        raise ValueError(f"empty tensor of shape {tuple(x.shape)}")
    sn, sc, sh, sw = x.stride()
    if w > 1 and sw != 1:
        raise ValueError("the innermost dimension must be contiguous (stride 1): interleaved pixels are not supported; "
                         "call .contiguous()")
    if (h > 1 and sh < w) or (c > 1 and sc <= 0) or (n > 1 and sn <= 0):
        raise ValueError(f"strides {tuple(x.stride())}: rows must not overlap and channel / frame strides must be positive")
    if x.device.type != "cuda":
        raise ValueError(f"expected a tensor on cuda:{device_index}, got one on {x.device} (there is no CPU path)")
    if x.device.index != device_index:
        raise ValueError(f"expected a tensor on cuda:{device_index}, got one on {x.device}")
    return n, h, w, (sh if h > 1 else w), (sc if c > 1 else 0), (sn if n > 1 else 0)


def _elem_of(dtype):
    import torch
    return {torch.float32: ELEM_F32, torch.float16: ELEM_F16, torch.bfloat16: ELEM_BF16, torch.uint8: ELEM_U8}.get(dtype)


def _u8_scale(name, scale, default):
    scale = default if scale is None else float(scale)
    if not (scale > 0.0 and scale != float("inf")):
        raise ValueError(f"{name} {scale!r}: expected a finite number > 0")
    return scale


def describe_image(x, channels: int, in_scale=None):
    """The Image of a tensor as it is stored: x is (N, C, H, W) or (C, H, W) with C = channels, dtype float32, float16, bfloat16
    or uint8, every stride of a dimension longer than 1 positive -- a permuted H x W x C view and a channels_last tensor have a
    pixel step of C and a channel pitch of 1.  Returns (image, n, h, w); ValueError otherwise.  Looks at shape, dtype and strides
    only: the device is check_image_device's."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"expected a torch.Tensor, got {type(x).__name__}")
    elem = _elem_of(x.dtype)
    if elem is None:
        raise ValueError(f"expected a float32, float16, bfloat16 or uint8 tensor, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"expected shape (N, {channels}, H, W) or ({channels}, H, W), got {tuple(x.shape)}")
    shape, strides = tuple(x.shape), tuple(x.stride())
    if x.dim() == 3:
        shape, strides = (1,) + shape, (0,) + strides
    n, c, h, w = shape
    if c != channels:
        raise ValueError(f"expected {channels} channel(s), the tensor has {c}: shape {tuple(x.shape)} (an H x W x C image goes in as "
                         "its view .permute(2, 0, 1))")
    if 0 in (n, h, w):
        raise ValueError(f"empty tensor of shape {tuple(x.shape)}")
    if any(count > 1 and step <= 0 for count, step in zip(shape, strides)):
        raise ValueError(f"strides {tuple(x.stride())}: every stride of a dimension longer than 1 must be positive")
    sn, sc, sh, sw = (step if count > 1 else 0 for count, step in zip(shape, strides))
    scale = _u8_scale("in_scale", in_scale, 1.0 / 255.0) if elem == ELEM_U8 else 1.0
    return Image(x.data_ptr(), elem, sw if w > 1 else 1, sh, sc, sn, scale), n, h, w


def check_image_device(x, device_index: int):
    if x.device.type != "cuda":
        raise ValueError(f"expected a tensor on cuda:{device_index}, got one on {x.device} (there is no CPU path)")
    if x.device.index != device_index:
        raise ValueError(f"expected a tensor on cuda:{device_index}, got one on {x.device}")


def is_channels_last(image: Image, channels: int) -> bool:
    """Whether the pixels of a described tensor are interleaved: the default layout of a call's result."""
    return channels > 1 and image.ch_pitch != 0 and image.ch_pitch < image.px_step


def empty_image(x, n, channels, h, w, dtype, channels_last, out_scale=None):
    """A new tensor for a call's result, shaped like x ((N, C, h, w), or (C, h, w) for a 3-dimensional x), and its Image:
    channels_last allocates N x h x w x C and returns the permuted view."""
    import torch
    elem = _elem_of(dtype)
    if elem is None:
        raise ValueError(f"out_dtype {dtype}: expected float32, float16, bfloat16 or uint8")
    scale = _u8_scale("out_scale", out_scale, 255.0) if elem == ELEM_U8 else 1.0
    if channels_last:
        out = torch.empty((n, h, w, channels), dtype=dtype, device=x.device).permute(0, 3, 1, 2)
        image = Image(out.data_ptr(), elem, channels, w * channels, 1, h * w * channels, scale)
    else:
        out = torch.empty((n, channels, h, w), dtype=dtype, device=x.device)
        image = Image(out.data_ptr(), elem, 1, w, h * w, channels * h * w, scale)
    return (out[0] if x.dim() == 3 else out), image


def check_size(size):
    """ValueError unless size is (H, W), two positive integers; returns them as ints."""
    try:
        dh, dw = size
    except (TypeError, ValueError):
        raise ValueError(f"size {size!r}: expected (H, W)") from None
    for v in (dh, dw):
        if isinstance(v, bool) or int(v) != v or v <= 0:
            raise ValueError(f"size {size!r}: expected two positive integers (H, W)")
    return int(dh), int(dw)


def check_antialias(antialias, plain, antialiased):
    """ValueError unless antialias is a bool; the name of the Context call it selects."""
    if not isinstance(antialias, bool):
        raise ValueError(f"antialias {antialias!r}: expected True or False")
    return antialiased if antialias else plain


class CompiledModule:
    """What compile_module returns: a callable that owns its Context (one GPU, the module's weights and padding)."""

    def __init__(self, ctx: Context, channels: int, device: int):
        self.ctx, self.channels, self.device = ctx, channels, device
        self._side = None

    def _on_current_stream(self, device, launch):
        """Run launch() -- calls on self.ctx -- as if on torch.cuda.current_stream(device).
        The library takes a stream handle and reads 0 as "the context's own stream", so torch's default stream (handle 0)
        cannot be handed over: the call then runs on a side stream of this callable, ordered after and before the default
        stream by events, which for the caller is the same as running on it."""
        import torch
        cur = torch.cuda.current_stream(device)
        run_on = cur
        if cur.cuda_stream == 0:
            if self._side is None:
                self._side = torch.cuda.Stream(device=device)
            run_on = self._side
            run_on.wait_stream(cur)
        self.ctx.set_stream(run_on.cuda_stream)
        launch()
        if run_on is not cur:
            cur.wait_stream(run_on)

    def __call__(self, x):
        import torch
        n, h, w, stride, ch_pitch, frame_pitch = check_input(x, self.channels, self.device)
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        self._on_current_stream(x.device, lambda: self.ctx.forward_f32_dev(
            x.data_ptr(), stride, ch_pitch, frame_pitch, out.data_ptr(), w, h * w, self.channels * h * w, w, h, n))
        return out

    def _resized(self, x, size, call):
        import torch
        n, h, w, stride, ch_pitch, frame_pitch = check_input(x, self.channels, self.device)
        dh, dw = check_size(size)
        out = torch.empty(tuple(x.shape[:-2]) + (dh, dw), dtype=torch.float32, device=x.device)
        self._on_current_stream(x.device, lambda: call(x.data_ptr(), stride, ch_pitch, frame_pitch, w, h, out.data_ptr(), dw,
                                                       dh * dw, self.channels * dh * dw, dw, dh, n))
        return out

    def resize(self, x, size, antialias=False):
        """F.interpolate(x, size=size, mode="bicubic", align_corners=False, antialias=antialias) with this library's kernels:
        size = (H, W) of the result.  The same tensors as __call__ takes, read where they lie, on the current stream.
        antialias=True is the resize that shrinks without aliasing (the degradation in front of an evaluation: hr -> lr)."""
        call = check_antialias(antialias, "resize_cubic_f32_dev", "resize_cubic_aa_f32_dev")
        return self._resized(x, size, lambda *a: getattr(self.ctx, call)(*a[:-1], self.channels, a[-1]))

    def upscale(self, x, scale=None, size=None):
        """module(F.interpolate(x, size, mode="bicubic", align_corners=False)): the bicubic resize of a low-resolution tensor
        and the module on the result, in one call and without a full-size intermediate tensor per batch.  Exactly one of
        scale (size = (int(h * scale), int(w * scale))) and size = (H, W) is given.  Equals self(self.resize(x, size))."""
        if (scale is None) == (size is None):
            raise ValueError("upscale: give exactly one of scale and size")
        if size is None:
            from . import scaled_size
            check_input(x, self.channels, self.device)
            ow, oh = scaled_size(int(x.shape[-1]), int(x.shape[-2]), float(scale))
            size = (oh, ow)
        return self._resized(x, size, lambda *a: self.ctx.process_f32_dev(*a))

    def upscale_rgb(self, x, scale=None, size=None, luma=LUMA_BT601, clamp=None):
        """A 1-channel module on the luma of a 3-channel tensor, the usual script around a luma SRCNN in one call: bicubic
        resize of the three planes, RGB -> Y'CbCr, the module on Y, Y'CbCr -> RGB, clamp.  x: float32 (N, 3, H, W) or (3, H, W)
        on the module's GPU, read where it lies; exactly one of scale and size = (H, W), never smaller than x (size equal to
        x's: an image that is already up-sampled).  luma = (w0, w1, w2, offset), the luma row of the colour convention for the
        planes in the order given (LUMA_BT601, luma_bt601_studio(), luma_for_order()); clamp = (lo, hi) or None.  Per plane
        the result is resize(x_c) + (module(Yup) - Yup) / (w0 + w1 + w2), Yup = resize(luma of x)."""
        import torch
        if self.channels != 1:
            raise ValueError(f"upscale_rgb runs a 1-channel module on the luma of the tensor: this module has {self.channels} "
                             "channels (upscale runs it on the planes themselves)")
        if (scale is None) == (size is None):
            raise ValueError("upscale_rgb: give exactly one of scale and size")
        n, h, w, stride, ch_pitch, frame_pitch = check_input(x, 3, self.device)
        if size is None:
            from . import scaled_size
            ow, oh = scaled_size(w, h, float(scale))
            size = (oh, ow)
        dh, dw = check_size(size)
        if dh < h or dw < w:
            raise ValueError(f"size {(dh, dw)} is smaller than the tensor's {(h, w)}: upscale_rgb resizes up or not at all")
        _luma4(luma), _clamp2(clamp)      # refused here, before anything is allocated or the library is reached
        out = torch.empty(tuple(x.shape[:-2]) + (dh, dw), dtype=torch.float32, device=x.device)
        self._on_current_stream(x.device, lambda: self.ctx.process_rgb_f32_dev(
            x.data_ptr(), stride, ch_pitch, frame_pitch, w, h, out.data_ptr(), dw, dh * dw, 3 * dh * dw, dw, dh, luma, clamp, n))
        return out

    # ---- images as they are stored: any of four dtypes, any positive strides, in and out ----
    def _image_call(self, x, channels, size, out_dtype, out_channels_last, in_scale, out_scale, call, check=None):
        src, n, h, w = describe_image(x, channels, in_scale)
        dh, dw = (h, w) if size is None else size(h, w)
        if check is not None:
            check(h, w, dh, dw)
        check_image_device(x, self.device)
        last = is_channels_last(src, channels) if out_channels_last is None else bool(out_channels_last) and channels > 1
        out, dst = empty_image(x, n, channels, dh, dw, x.dtype if out_dtype is None else out_dtype, last, out_scale)
        self._on_current_stream(x.device, lambda: call(src, w, h, dst, dw, dh, n))
        return out

    @staticmethod
    def _target(name, scale, size):
        if (scale is None) == (size is None):
            raise ValueError(f"{name}: give exactly one of scale and size")
        if size is not None:
            dh, dw = check_size(size)
            return lambda h, w: (dh, dw)
        from . import scaled_size
        return lambda h, w: scaled_size(w, h, float(scale))[::-1]

    def forward_image(self, x, out_dtype=None, out_channels_last=None, in_scale=None, out_scale=None):
        """self(x) on a tensor as it is stored: float32, float16, bfloat16 or uint8, any positive strides (pass an H x W x C
        image as its view .permute(2, 0, 1)), read where it lies.  The result has out_dtype (default: x's) and is channels-last
        where out_channels_last says so (default: where x is).  uint8 is read as byte * in_scale (default 1 / 255) and written
        as round(clamp(value * out_scale, 0, 255)) (default 255).  Bit for bit store(self(load(x)))."""
        return self._image_call(x, self.channels, None, out_dtype, out_channels_last, in_scale, out_scale,
                                lambda s, w, h, d, dw, dh, n: self.ctx.forward_image_dev(s, d, w, h, n))

    def resize_image(self, x, size, out_dtype=None, out_channels_last=None, in_scale=None, out_scale=None, antialias=False):
        """resize() on a tensor as it is stored (see forward_image); size equal to x's converts the format and nothing else
        (with antialias=False)."""
        call = check_antialias(antialias, "resize_cubic_image_dev", "resize_cubic_aa_image_dev")
        dh, dw = check_size(size)
        return self._image_call(x, self.channels, lambda h, w: (dh, dw), out_dtype, out_channels_last, in_scale, out_scale,
                                lambda s, w, h, d, dw, dh, n: getattr(self.ctx, call)(s, w, h, d, dw, dh, self.channels, n))

    def upscale_image(self, x, scale=None, size=None, out_dtype=None, out_channels_last=None, in_scale=None, out_scale=None):
        """upscale() on a tensor as it is stored (see forward_image)."""
        return self._image_call(x, self.channels, self._target("upscale_image", scale, size), out_dtype, out_channels_last, in_scale,
                                out_scale, lambda *a: self.ctx.process_image_dev(*a))

    def upscale_rgb_image(self, x, scale=None, size=None, luma=LUMA_BT601, clamp=None, out_dtype=None, out_channels_last=None,
                          in_scale=None, out_scale=None):
        """upscale_rgb() on a tensor as it is stored (see forward_image): a decoded H x W x 3 uint8 picture goes in as
        .permute(2, 0, 1) and comes back as uint8 at the target size, the same view of an H' x W' x 3 tensor.  luma and clamp
        are in the units of the LOADED values ([0, 1] for uint8 with the default in_scale); the clamp applies in float32,
        ahead of the store."""
        if self.channels != 1:
            raise ValueError(f"upscale_rgb_image runs a 1-channel module on the luma of the tensor: this module has {self.channels} "
                             "channels (upscale_image runs it on the channels themselves)")
        target = self._target("upscale_rgb_image", scale, size)

        def check(h, w, dh, dw):
            if dh < h or dw < w:
                raise ValueError(f"size {(dh, dw)} is smaller than the tensor's {(h, w)}: upscale_rgb_image resizes up or not at all")
            _luma4(luma), _clamp2(clamp)
        return self._image_call(x, 3, target, out_dtype, out_channels_last, in_scale, out_scale,
                                lambda *a: self.ctx.process_rgb_image_dev(*a[:-1], luma, clamp, a[-1]), check)

    # ---- Pillow's resize of uint8 tensors, byte for byte ----
    @staticmethod
    def _pil_filter(name, x, filter):
        """The SRCNN_PIL_* number of filter ("bilinear" or "bicubic"); TypeError for a tensor that is not uint8"""
        import torch
        from . import PIL_FILTERS
        if isinstance(x, torch.Tensor) and x.dtype != torch.uint8:
            raise TypeError(f"{name} takes a uint8 tensor, as Pillow's Image.resize takes an 8-bit picture; this one is {x.dtype}: "
                            "a float tensor is resized by resize(..., antialias=True)")
        if not isinstance(filter, str) or filter not in PIL_FILTERS:
            raise ValueError(f"filter {filter!r}: expected one of {sorted(PIL_FILTERS)}")
        return PIL_FILTERS[filter]

    def resize_pil(self, x, size, filter="bicubic"):
        """Image.resize((W, H), Image.BICUBIC or Image.BILINEAR) of Pillow on a uint8 tensor, byte for byte: the picture a
        Pillow-based training or test script makes, up, down or at the same size.  x: uint8 (N, C, H, W) or (C, H, W) on the
        module's GPU with any number of channels and any positive strides (channels_last, a permuted H x W x C view), read
        where it lies; size = (H, W).  Returns uint8 in the same memory format.  Runs on the current stream."""
        import torch
        f = self._pil_filter("resize_pil", x, filter)
        if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
            raise ValueError(f"expected a uint8 tensor of shape (N, C, H, W) or (C, H, W), got {getattr(x, 'shape', type(x).__name__)}")
        channels = int(x.shape[-3])
        dh, dw = check_size(size)
        return self._image_call(x, channels, lambda h, w: (dh, dw), None, None, None, None,
                                lambda s, w, h, d, dw, dh, n: self.ctx.resize_pil_image_dev(s, w, h, d, dw, dh, channels, n, f))

    def upscale_pil(self, x, scale=None, size=None, filter="bicubic", out_dtype=None, out_channels_last=None, in_scale=None,
                    out_scale=None):
        """The module on Pillow's resize of a uint8 tensor: forward_image(resize_pil(x, size, filter)) in one call, bit for
        bit -- what a script does that builds its input with Image.resize and ToTensor.  x: uint8 with the module's channels;
        the resized bytes are read as byte * in_scale (default 1 / 255); out_dtype (default uint8), out_channels_last and
        out_scale as forward_image takes them.  Never shrinks."""
        f = self._pil_filter("upscale_pil", x, filter)

        def check(h, w, dh, dw):
            if dh < h or dw < w:
                raise ValueError(f"size {(dh, dw)} is smaller than the tensor's {(h, w)}: upscale_pil resizes up or not at all")
        return self._image_call(x, self.channels, self._target("upscale_pil", scale, size), out_dtype, out_channels_last, in_scale,
                                out_scale, lambda *a: self.ctx.process_pil_image_dev(*a, f), check)

    def upscale_rgb_pil(self, x, scale=None, size=None, luma=LUMA_BT601, clamp=None, out_dtype=None, out_channels_last=None,
                        in_scale=None, out_scale=None, filter="bicubic"):
        """upscale_rgb_image(resize_pil(x, size, filter), size=size) in one call, bit for bit: a 1-channel module on the luma of
        a uint8 RGB tensor that Pillow's resize has brought to the target size.  The arguments of upscale_rgb_image, and filter."""
        f = self._pil_filter("upscale_rgb_pil", x, filter)
        if self.channels != 1:
            raise ValueError(f"upscale_rgb_pil runs a 1-channel module on the luma of the tensor: this module has {self.channels} "
                             "channels (upscale_pil runs it on the channels themselves)")
        target = self._target("upscale_rgb_pil", scale, size)

        def check(h, w, dh, dw):
            if dh < h or dw < w:
                raise ValueError(f"size {(dh, dw)} is smaller than the tensor's {(h, w)}: upscale_rgb_pil resizes up or not at all")
            _luma4(luma), _clamp2(clamp)
        return self._image_call(x, 3, target, out_dtype, out_channels_last, in_scale, out_scale,
                                lambda *a: self.ctx.process_rgb_pil_image_dev(*a[:-1], luma, clamp, a[-1], f), check)

    # ---- full-reference metrics: the measurement at the end of an evaluation ----
    @staticmethod
    def _metric_args(a, b, border, luma, data_range, in_scale, early=None):
        """What metrics() and msssim_sums() check alike, in one order: -> (ia, ib, n, channels, h, w, rh, rw, data_range)"""
        import math
        import torch
        from . import _metric_luma4
        if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
            raise ValueError(f"expected two torch.Tensors, got {type(a).__name__} and {type(b).__name__}")
        if a.dim() not in (3, 4) or tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"expected two tensors of the same shape (N, C, H, W) or (C, H, W), got {tuple(a.shape)} and {tuple(b.shape)}")
        channels = int(a.shape[-3])
        if channels not in (1, 3):
            raise ValueError(f"expected 1 or 3 channels, the tensors have {channels}: shape {tuple(a.shape)}")
        ia, n, h, w = describe_image(a, channels, in_scale)
        ib = describe_image(b, channels, in_scale)[0]
        if early is not None:
            early()
        if isinstance(border, bool) or not isinstance(border, int) or border < 0:
            raise ValueError(f"border {border!r}: expected an integer >= 0")
        if luma is not None and channels != 3:
            raise ValueError(f"luma needs 3 channels, the tensors have {channels} (luma=None measures the plane itself)")
        _metric_luma4(luma)
        try:
            data_range = float(data_range)
        except (TypeError, ValueError):
            raise ValueError(f"data_range {data_range!r}: expected a finite number > 0") from None
        if not (data_range > 0.0 and math.isfinite(data_range)):
            raise ValueError(f"data_range {data_range!r}: expected a finite number > 0")
        rh, rw = h - 2 * border, w - 2 * border
        if rh < 1 or rw < 1:
            raise ValueError(f"a border of {border} leaves nothing of a {h} x {w} picture")
        return ia, ib, n, channels, h, w, rh, rw, data_range

    def metrics(self, a, b, border=0, luma=None, data_range=1.0, ssim=True, in_scale=None):
        """The raw sums behind PSNR and SSIM of two pictures as they are stored: a float64 CUDA tensor (N, P, 4) holding
        (sse, n_px, ssim_sum, n_win) per frame and result.  a and b: (N, C, H, W) or (C, H, W) of the same shape with C = 1 or 3
        (taken from the tensors, not from the module), each float32, float16, bfloat16 or uint8 with any positive strides;
        they may differ in dtype and layout.  uint8 is read as byte * in_scale (default 1 / 255).  border rows and columns are
        shaved off every side first.  luma = (w0, w1, w2, offset) measures the luma of 3-channel pictures (P = 1); None
        measures every channel plane (P = C).  data_range is L of the SSIM constants, in loaded units.  ssim=False computes
        the squared error only (the SSIM fields are then 0).  Float64 after the load, no atomics: the same bits every time.
        Runs on the current stream, with no synchronisation."""
        import torch
        from . import METRIC_SSE, METRIC_SSIM

        def early():
            if not isinstance(ssim, bool):
                raise ValueError(f"ssim {ssim!r}: expected True or False")
        ia, ib, n, channels, h, w, rh, rw, data_range = self._metric_args(a, b, border, luma, data_range, in_scale, early)
        if ssim and (rh < 11 or rw < 11):
            raise ValueError(f"SSIM needs a region of at least 11 x 11, this one is {rh} x {rw} (ssim=False measures the squared error alone)")
        check_image_device(a, self.device)
        check_image_device(b, self.device)
        per_frame = 1 if luma is not None else channels
        out = torch.empty((n, per_frame, 4), dtype=torch.float64, device=a.device)
        flags = METRIC_SSE | (METRIC_SSIM if ssim else 0)
        self._on_current_stream(a.device, lambda: self.ctx.metrics_image_dev(ia, ib, w, h, channels, n, border, luma, data_range, flags,
                                                                             out.data_ptr()))
        return out

    def psnr(self, a, b, border=0, luma=None, data_range=1.0, in_scale=None):
        """10 log10(L^2 n_px / sse) per frame and result from metrics(): a float64 CUDA tensor (N, P), inf where the pictures
        are equal.  Torch operations on the device, no synchronisation."""
        import torch
        m = self.metrics(a, b, border=border, luma=luma, data_range=data_range, ssim=False, in_scale=in_scale)
        return 10.0 * torch.log10((float(data_range) ** 2) * m[..., 1] / m[..., 0])

    def ssim(self, a, b, border=0, luma=None, data_range=1.0, in_scale=None):
        """Mean SSIM (11-tap Gaussian window, sigma 1.5, valid windows) per frame and result from metrics(): a float64 CUDA
        tensor (N, P)."""
        m = self.metrics(a, b, border=border, luma=luma, data_range=data_range, ssim=True, in_scale=in_scale)
        return m[..., 2] / m[..., 3]

    def msssim_sums(self, a, b, border=0, luma=None, data_range=1.0, n_scales=5, in_scale=None):
        """The raw sums behind MS-SSIM of two pictures as they are stored: a float64 CUDA tensor (N, P, n_scales, 3) holding
        (cs_sum, ssim_sum, n_win) per frame, result and scale.  a, b, luma, data_range and in_scale as metrics() takes them.
        border is shaved off at scale 0 only; scale j + 1 is the 2 x 2 mean of scale j, an odd last row or column paired with
        itself.  n_scales: 1 .. 5; the region must be at least 10 * 2^(n_scales - 1) + 1 on a side (161 for five).  Float64
        after the load, no atomics: the same bits every time.  Runs on the current stream, with no synchronisation."""
        import torch
        from . import MSSSIM_MAX_SCALES
        ia, ib, n, channels, h, w, rh, rw, data_range = self._metric_args(a, b, border, luma, data_range, in_scale)
        if isinstance(n_scales, bool) or not isinstance(n_scales, int) or not 1 <= n_scales <= MSSSIM_MAX_SCALES:
            raise ValueError(f"n_scales {n_scales!r}: expected an integer 1 .. {MSSSIM_MAX_SCALES}")
        least = 10 * 2 ** (n_scales - 1) + 1
        if rh < least or rw < least:
            raise ValueError(f"{n_scales} scales need a region of at least {least} x {least}, this one is {rh} x {rw}")
        check_image_device(a, self.device)
        check_image_device(b, self.device)
        out = torch.empty((n, 1 if luma is not None else channels, n_scales, 3), dtype=torch.float64, device=a.device)
        self._on_current_stream(a.device, lambda: self.ctx.msssim_image_dev(ia, ib, w, h, channels, n, border, luma, data_range, n_scales,
                                                                            out.data_ptr()))
        return out

    def msssim(self, a, b, border=0, luma=None, data_range=1.0, n_scales=5, weights=None, in_scale=None):
        """MS-SSIM per frame and result from msssim_sums(): a float64 CUDA tensor (N, P), the product over the scales of
        max(mean, 0)^w with the mean of cs below the last scale and of ssim at it (0 where a mean is not positive).
        weights=None: those of Wang, Simoncelli and Bovik, which needs n_scales=5.  Torch operations on the device, no
        synchronisation."""
        import math
        import torch
        from . import MSSSIM_WEIGHTS
        if weights is None:
            if n_scales != len(MSSSIM_WEIGHTS):
                raise ValueError(f"weights=None means the five published weights: n_scales {n_scales!r} needs weights of its own")
            weights = MSSSIM_WEIGHTS
        try:
            wl = [float(v) for v in weights]
        except (TypeError, ValueError):
            raise ValueError(f"weights {weights!r}: expected n_scales numbers") from None
        if len(wl) != n_scales or any(math.isnan(v) for v in wl):
            raise ValueError(f"weights {weights!r}: expected {n_scales!r} numbers, none a NaN")
        m = self.msssim_sums(a, b, border=border, luma=luma, data_range=data_range, n_scales=n_scales, in_scale=in_scale)
        mean = torch.cat((m[..., :-1, 0], m[..., -1:, 1]), dim=-1) / m[..., 2]
        out = None
        for s, ws in enumerate(wl):      # (the weights stay Python numbers: no copy to the device)
            ms = mean[..., s]
            factor = torch.where(ms > 0, ms.clamp_min(0.0).pow(ws), torch.zeros_like(ms))
            out = factor if out is None else out * factor
        return out

    def close(self):
        self.ctx.close()


def compile_module(module, device: int = 0, mode: int = MODE_MFMA, input_range: float = 1.0) -> CompiledModule:
    """An SRCNN nn.Module (conv1 9x9, conv2 f2 x f2 with f2 = 1, 3, 5, conv3 5x5; 1 or 3 channels; every layer padded by k // 2
    with padding_mode "zeros" or "replicate") -> a callable on float32 CUDA tensors that computes module(x) with this library's
    HIP kernels.  mode: MODE_MFMA (float32 throughout) or MODE_BANDED16 (layer 2 in split f16, faster; input_range is then the
    largest |x| the tensors will hold, 1.0 for [0, 1] data).  The weights are read once, here: a module trained further needs a
    new compile_module.  The filters: conv1 up to 128, conv2 up to 64 (64 / 32 is the classic model).  MODE_BANDED16 is the
    fast mode for every width: a module wider than 64 / 32 keeps its context in MODE_MFMA, the only mode that runs such a model,
    with Context.set_wide_split16(True) -- the same split-f16 layer 2, the same input_range."""
    if mode not in (MODE_MFMA, MODE_BANDED16):
        raise ValueError(f"mode {mode}: the float image path runs in MODE_MFMA and MODE_BANDED16 only")
    conv1 = getattr(module, "conv1", None)
    if conv1 is None:
        raise ValueError("module has no conv1")
    channels = int(conv1.in_channels)
    if channels not in (1, 3):
        raise ValueError(f"conv1 reads {channels} channels: a model has 1 channel or 3")
    model, padding = model_from_module(module, input_scale=1.0, image_order="rgb" if channels == 3 else None)
    ctx = Context(int(device))
    try:
        ctx.set_model(*model)
        ctx.set_padding(padding)
        _, n1, _, n2 = ctx.model_shape()
        if mode == MODE_BANDED16 and (n1 > 64 or n2 > 32):
            ctx.set_mode(MODE_MFMA)
            ctx.set_wide_split16(True)
        else:
            ctx.set_mode(mode)
        ctx.set_input_range(input_range)
    except Exception:
        ctx.close()
        raise
    return CompiledModule(ctx, channels, int(device))
