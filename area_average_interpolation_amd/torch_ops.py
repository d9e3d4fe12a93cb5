"""The resampling as a differentiable torch operator.

``resample(x, ...)`` runs the library's forward (aai_resample_batch_device_f32) on a device-resident fp32 tensor and is a
``torch.autograd.Function``: its backward is the library's adjoint (aai_adjoint_batch_device_f32), gsrc = W^T gdst with the
forward's own weights -- not an approximation through ``grid_sample`` (``planned_backward=True``: the planned adjoint,
aai_adjoint_planned_batch_device_f32; ``"any"``: aai_adjoint_rotated_batch_device_f32, planned at every rotation; ``"interleaved"``:
``"any"`` plus aai_adjoint_rotated_interleaved_device_f32 for channels_last tensors at general rotations; ``"channels_last"``:
``"interleaved"`` plus aai_adjoint_planned_interleaved_device_f32 for channels_last tensors at multiples of 90 degrees).  Both launch on ``torch.cuda.current_stream()`` of the
tensor's device and only enqueue work.  ``sampler_backward=True`` makes the bilinear / bicubic modes differentiable as well: their backward
is aai_adjoint_sample_batch_device_f32 (aai_adjoint_sample_interleaved_device_f32 for channels_last tensors).  ``f64=True`` is the
reference-precision operator on float64 tensors (aai_resample_batch_device_f64 / aai_adjoint_batch_device_f64): differentiable to any order.
``half=True`` takes float16 / bfloat16 tensors and returns the same dtype (aai_resample_half_batch_device); its backward widens the
gradient, runs the fp32 adjoint and rounds once.  ``half="channels_last"`` additionally reads a channels_last float16 / bfloat16
(B, C, H, W) tensor with 2 <= C <= 4 in place (aai_resample_half_interleaved_device) and returns a channels_last tensor.

torch is imported here, not by the package: ``import area_average_interpolation_amd`` works without it.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from . import api


def _ensure_prepared(rq, channels=1):
    """The forward's first call per (geometry, channel count, device) builds a plan and synchronises (aai_prepare): do that now,
    outside any stream capture.  Inside a capture an unprepared geometry is an error, not a hidden synchronisation."""
    if api.plan_shape(rq, channels):
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("resample(): this geometry has no plan on this device yet and the current stream is being captured; "
                           "call resample() (or prepare()) once with the same geometry before capturing")
    api.prepare(rq, channels)


# route of resample()'s backward -> (tokens of api.plan_shape(rq) -> are the plan's adjoint tables still to be built?, what builds them,
# planned_backward as the message shows it)
#   planned      planned_backward=True, or "any" at a multiple of 90 degrees: only a separable (kernel=1), non-dense plan can hold such tables;
#                every other plan's backward runs the general kernels, which need none
#   rotated      "any" at a general rotation: the plan's sums and knife lists
#   interleaved  the tables of aai_adjoint_rotated_interleaved_device_f32 live on the SINGLE-channel plan of the geometry, which the
#                interleaved forward (prepared for C channels) does not build: aai_adjoint_rotated_prepare builds both
#   separable    the tables of aai_adjoint_planned_interleaved_device_f32 at a multiple of 90 degrees are those of "planned", and they too
#                live on the SINGLE-channel plan (plan_shape(rq, 1)), which the interleaved forward does not build: missing while that plan
#                is missing or says adjoint=none; aai_adjoint_rotated_prepare builds the plan and the tables
_ADJOINT_TABLES = {
    "planned": (lambda t: "kernel=%d" % L.KERNEL_AXIS in t and "dense=0" in t and "adjoint=none" in t, api.adjoint_prepare, "True"),
    "rotated": (lambda t: "rot_adjoint=none" in t, api.adjoint_rotated_prepare, '"any"'),
    "interleaved": (lambda t: not t or "rot_adjoint=none" in t, api.adjoint_rotated_prepare, '"interleaved"'),
    "separable": (lambda t: not t or ("kernel=%d" % L.KERNEL_AXIS in t and "dense=0" in t and "adjoint=none" in t), api.adjoint_rotated_prepare,
                  '"channels_last"'),
}


def _ensure_adjoint_prepared(rq, route, asked=None):
    """The first call of a planned adjoint per (geometry, device) builds the plan's adjoint tables and synchronises (aai_adjoint_prepare,
    aai_adjoint_rotated_prepare): do that in the forward, outside any stream capture.  Inside a capture missing tables are an error,
    not a hidden synchronisation."""
    missing, prepare, shown = _ADJOINT_TABLES[route]
    if not missing(api.plan_shape(rq, 1).split()):
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("resample(%s): this geometry has no adjoint tables on this device yet and the current "
                           "stream is being captured; call resample() (or %s()) once with the same geometry before capturing"
                           % (asked or "planned_backward=%s" % shown, prepare.__name__))
    prepare(rq)


def _normalise_planned(planned_backward):
    """False | True | "any" | "interleaved" | "channels_last" (anything else that is a string raises)"""
    if isinstance(planned_backward, str):
        if planned_backward not in ("any", "interleaved", "channels_last"):
            raise ValueError('planned_backward must be False, True, "any", "interleaved" or "channels_last", got %r' % (planned_backward,))
        return planned_backward
    return bool(planned_backward)


# ctx.planned of a bilinear / bicubic request whose backward is the samplers' adjoint (sampler_backward=True): no plan, no tables
_SAMPLER = "sampler"


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rq, lay, planned):
        B, H, W = x.shape
        y = torch.empty((B, lay.dst_height, lay.dst_width), dtype=torch.float32, device=x.device)
        ctx.rq, ctx.src_shape, ctx.planned = rq, (B, H, W), planned
        if B:
            with torch.cuda.device(x.device):
                _ensure_prepared(rq)
                if planned and planned != _SAMPLER and ctx.needs_input_grad[0]:
                    _ensure_adjoint_prepared(rq, "rotated" if planned == "any" and lay.kernel in (L.KERNEL_ROTATED, L.KERNEL_FAST) else "planned")
                api.resample_device(rq, x.data_ptr(), W, y.data_ptr(), lay.dst_width, stream=torch.cuda.current_stream().cuda_stream,
                                    batch=B, src_image_stride=H * W, dst_image_stride=lay.dst_height * lay.dst_width)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _adjoint_f32(ctx.rq, ctx.src_shape, ctx.planned, gy), None, None, None


def _adjoint_f32(rq, src_shape, planned, gy):
    """gx (fp32, (B, H, W)) = W^T gy for a (B, dH, dW) gradient of any float dtype: the backward of _Resample and, widened, of _ResampleHalf"""
    B, H, W = src_shape
    gy = gy.contiguous()
    if gy.dtype != torch.float32:
        gy = gy.float()
    gx = torch.empty((B, H, W), dtype=torch.float32, device=gy.device)
    if B:
        dH, dW = gy.shape[1], gy.shape[2]
        with torch.cuda.device(gy.device):
            if planned == _SAMPLER:
                api.adjoint_sample_device(rq, gy.data_ptr(), dW, gx.data_ptr(), W, stream=torch.cuda.current_stream().cuda_stream,
                                          batch=B, dst_image_stride=dH * dW, src_image_stride=H * W)
            else:
                api.adjoint_device(rq, gy.data_ptr(), dW, gx.data_ptr(), W, stream=torch.cuda.current_stream().cuda_stream,
                                   batch=B, dst_image_stride=dH * dW, src_image_stride=H * W, planned=planned)
    return gx


_HALF_DTYPES = {torch.float16: L.HALF_F16, torch.bfloat16: L.HALF_BF16}


class _ResampleHalf(torch.autograd.Function):
    """y = round(W x) on a contiguous float16 / bfloat16 (B, H, W) tensor: aai_resample_half_batch_device, y in x's dtype.  The plan is the
    fp32 forward's.  Backward: gy widened to fp32, _Resample's adjoint (planned honoured the same way), the gradient rounded to x's dtype."""

    @staticmethod
    def forward(ctx, x, rq, lay, planned):
        B, H, W = x.shape
        y = torch.empty((B, lay.dst_height, lay.dst_width), dtype=x.dtype, device=x.device)
        ctx.rq, ctx.src_shape, ctx.planned, ctx.dtype = rq, (B, H, W), planned, x.dtype
        if B:
            with torch.cuda.device(x.device):
                _ensure_prepared(rq)
                if planned and planned != _SAMPLER and ctx.needs_input_grad[0]:
                    _ensure_adjoint_prepared(rq, "rotated" if planned == "any" and lay.kernel in (L.KERNEL_ROTATED, L.KERNEL_FAST) else "planned")
                api.resample_half_device(rq, x.data_ptr(), W, y.data_ptr(), lay.dst_width, _HALF_DTYPES[x.dtype],
                                         stream=torch.cuda.current_stream().cuda_stream, batch=B, src_image_stride=H * W,
                                         dst_image_stride=lay.dst_height * lay.dst_width)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _adjoint_f32(ctx.rq, ctx.src_shape, ctx.planned, gy).to(ctx.dtype), None, None, None


class _ResampleHalfInterleaved(torch.autograd.Function):
    """y = round(W x) on a float16 / bfloat16 (B, C, H, W) tensor dense in torch.channels_last, 2 <= C <= 4: the NHWC storage is the library's
    interleaved layout, aai_resample_half_interleaved_device reads it in place and y is channels_last in x's dtype.  The plan is the fp32
    interleaved forward's.  Backward: gy widened to fp32, the backward the fp32 operator runs for a channels_last tensor under the same
    planned_backward / sampler_backward (_nchw_route: `interleaved` and `planned` are its answer), the gradient rounded once to x's
    dtype, channels_last."""

    @staticmethod
    def forward(ctx, x, rq, lay, interleaved, planned):
        B, C, H, W = x.shape
        dH, dW = lay.dst_height, lay.dst_width
        y = torch.empty((B, C, dH, dW), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        ctx.rq, ctx.lay, ctx.src_shape, ctx.interleaved, ctx.planned, ctx.dtype = rq, lay, (B, C, H, W), interleaved, planned, x.dtype
        with torch.cuda.device(x.device):
            _ensure_prepared(rq, C)
            if planned and planned != _SAMPLER and ctx.needs_input_grad[0]:
                if interleaved:
                    _ensure_adjoint_prepared(rq, "separable" if planned == "separable" else "interleaved")
                else:
                    _ensure_prepared(rq)         # the planar backward runs on the single-channel plan
                    _ensure_adjoint_prepared(rq, "rotated" if planned == "any" and lay.kernel in (L.KERNEL_ROTATED, L.KERNEL_FAST) else "planned")
            api.resample_half_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C, _HALF_DTYPES[x.dtype],
                                                 stream=torch.cuda.current_stream().cuda_stream, batch=B, src_image_stride=H * W * C,
                                                 dst_image_stride=dH * dW * C)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        B, C, H, W = ctx.src_shape
        if ctx.interleaved:
            gx = _adjoint_interleaved_f32(ctx.rq, ctx.src_shape, ctx.planned, gy)
        else:
            gx = _adjoint_f32(ctx.rq, (B * C, H, W), ctx.planned, gy.contiguous().view(B * C, gy.shape[2], gy.shape[3])).view(B, C, H, W)
        return gx.to(ctx.dtype, memory_format=torch.channels_last), None, None, None, None


class _ResampleHalfNarrowBackward(torch.autograd.Function):
    """resample(..., half=..., half_backward=True): the forward of _ResampleHalf (x a contiguous (B, H, W) tensor, interleaved=False) or of
    _ResampleHalfInterleaved (x a (B, C, H, W) tensor dense in channels_last, interleaved=True), and a backward that stays in x's dtype:
    gy goes straight to aai_adjoint_half_device (include/aai_adjoint_half.h) and its output is x.grad -- no fp32 copy of gy, no fp32 gx,
    no conversion.  The gradient has the bits of the widening backward under planned_backward="any" (planar) / "channels_last"
    (interleaved): narrow(fp32 planned adjoint(widen(gy)))."""

    @staticmethod
    def forward(ctx, x, rq, lay, interleaved):
        B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        C = x.shape[1] if interleaved else 1
        dH, dW = lay.dst_height, lay.dst_width
        if interleaved:
            y = torch.empty((B, C, dH, dW), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        else:
            y = torch.empty((B, dH, dW), dtype=x.dtype, device=x.device)
        ctx.rq, ctx.src_shape, ctx.interleaved, ctx.dtype = rq, tuple(x.shape), interleaved, x.dtype
        if dH and dW:
            with torch.cuda.device(x.device):
                _ensure_prepared(rq, C)
                if ctx.needs_input_grad[0]:
                    # the adjoint tables live on the single-channel plan: at multiples of 90 degrees those of the transposed separable kernel,
                    # at a general rotation the sums of the forwarding route's planned adjoint (aai_adjoint_rotated_prepare builds either)
                    _ensure_adjoint_prepared(rq, "interleaved" if lay.kernel in (L.KERNEL_ROTATED, L.KERNEL_FAST) else "separable", "half_backward=True")
                api.resample_half_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C, _HALF_DTYPES[x.dtype],
                                                     stream=torch.cuda.current_stream().cuda_stream, batch=B, src_image_stride=H * W * C,
                                                     dst_image_stride=dH * dW * C)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        B, H, W = ctx.src_shape[0], ctx.src_shape[-2], ctx.src_shape[-1]
        C = ctx.src_shape[1] if ctx.interleaved else 1
        dH, dW = gy.shape[-2], gy.shape[-1]
        if gy.dtype != ctx.dtype:
            gy = gy.to(ctx.dtype)
        gy = gy.contiguous(memory_format=torch.channels_last) if ctx.interleaved else gy.contiguous()
        if not (dH and dW):
            return torch.zeros(ctx.src_shape, dtype=ctx.dtype, device=gy.device), None, None, None
        gx = torch.empty(ctx.src_shape, dtype=ctx.dtype, device=gy.device, memory_format=torch.channels_last if ctx.interleaved else torch.contiguous_format)
        with torch.cuda.device(gy.device):
            api.adjoint_half_device(ctx.rq, C, gy.data_ptr(), dW * C, gx.data_ptr(), W * C, _HALF_DTYPES[ctx.dtype],
                                    stream=torch.cuda.current_stream().cuda_stream, batch=B, dst_image_stride=dH * dW * C, src_image_stride=H * W * C)
        return gx, None, None, None


def _resample_half(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy, planned, sampler_backward, channels_last=False, half_backward=False):
    """resample(..., half=True): float16 / bfloat16 tensors in, the same dtype out (include/aai_half.h); channels_last: half="channels_last",
    the zero-copy route of include/aai_half_interleaved.h for the tensors that qualify"""
    if x.dtype not in _HALF_DTYPES:
        raise TypeError("resample(half=True) takes a float16 or bfloat16 tensor, got %s" % x.dtype)
    if x.dim() not in (2, 3, 4):
        raise ValueError("resample() takes a tensor of shape (H, W), (B, H, W) or (B, C, H, W)")
    if not x.is_cuda:
        raise ValueError("resample() takes a tensor on a GPU (the library has no CPU path)")
    H, W = x.shape[-2], x.shape[-1]
    rq, lay = _query(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    iso = (lay.dst_iso_x, lay.dst_iso_y)
    lead = tuple(x.shape[:-2])
    if 0 in lead:
        return torch.empty(lead + (lay.dst_height, lay.dst_width), dtype=x.dtype, device=x.device), iso
    sampler = mode not in (L.MODE_AREA, L.MODE_FAST)
    if x.requires_grad and torch.is_grad_enabled() and sampler and not sampler_backward:
        raise ValueError(_NO_SAMPLER_ADJOINT)
    if (channels_last and x.dim() == 4 and 2 <= x.shape[1] <= 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
            and lay.dst_height > 0 and lay.dst_width > 0):
        if half_backward:
            return _ResampleHalfNarrowBackward.apply(x, rq, lay, True), iso
        return _ResampleHalfInterleaved.apply(x, rq, lay, *_nchw_route(True, lay, mode, planned, sampler_backward)), iso
    if planned in ("interleaved", "channels_last"):
        planned = "any"              # the half=True path has no interleaved route
    if sampler and sampler_backward:
        planned = _SAMPLER
    # every rank through the (B, H, W) operator; a 4-D tensor plane by plane (channels_last and other strided input is made contiguous)
    if half_backward:
        y = _ResampleHalfNarrowBackward.apply(x.contiguous().view(-1, H, W), rq, lay, False)
    else:
        y = _ResampleHalf.apply(x.contiguous().view(-1, H, W), rq, lay, planned)
    return y.view(lead + (lay.dst_height, lay.dst_width)), iso


_INT_DTYPES = {torch.uint8: L.DTYPE_U8}
if hasattr(torch, "uint16"):
    _INT_DTYPES[torch.uint16] = L.DTYPE_U16


def _resample_int(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy):
    """resample(..., integer=True): uint8 / uint16 tensors in, the same dtype out (include/aai_int.h); no autograd"""
    if x.dtype not in _INT_DTYPES:
        raise TypeError("resample(integer=True) takes a uint8 or uint16 tensor, got %s" % x.dtype)
    if x.dim() not in (2, 3, 4):
        raise ValueError("resample() takes a tensor of shape (H, W), (B, H, W) or (B, C, H, W)")
    if not x.is_cuda:
        raise ValueError("resample() takes a tensor on a GPU (the library has no CPU path)")
    if x.dim() == 4 and x.shape[1] > 4:
        raise ValueError("resample(integer=True) takes at most 4 channels, got %d" % x.shape[1])
    H, W = x.shape[-2], x.shape[-1]
    rq, lay = _query(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    iso = (lay.dst_iso_x, lay.dst_iso_y)
    dH, dW = lay.dst_height, lay.dst_width
    lead = tuple(x.shape[:-2])
    x = x.detach()
    # (B, C, H, W) dense in channels_last with C > 1: the NHWC storage is the library's interleaved layout, nothing is copied
    interleaved = x.dim() == 4 and x.shape[1] > 1 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    if interleaved:
        y = torch.empty(lead + (dH, dW), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        images, C = x.shape[0], x.shape[1]
    else:
        x = x.contiguous()
        y = torch.empty(lead + (dH, dW), dtype=x.dtype, device=x.device)
        images, C = x.numel() // max(H * W, 1), 1
    if 0 in lead or dH == 0 or dW == 0:
        return y, iso
    with torch.cuda.device(x.device):
        _ensure_prepared(rq, C)
        api.resample_int_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C, _INT_DTYPES[x.dtype], stream=torch.cuda.current_stream().cuda_stream,
                                batch=images, src_image_stride=H * W * C, dst_image_stride=dH * dW * C)
    return y, iso


_CONVERT_DTYPES = {torch.float32: L.DTYPE_F32, torch.float16: L.HALF_F16, torch.bfloat16: L.HALF_BF16}


def _resample_convert(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy, out_dtype, scale, offset, out_memory_format):
    """resample(..., integer=True, out_dtype=...): uint8 / uint16 tensors in, a scaled float32 / float16 / bfloat16 tensor out, written by
    the library in its final memory format (include/ext/aai_convert.h); no autograd"""
    if x.dtype not in _INT_DTYPES:
        raise TypeError("resample(integer=True) takes a uint8 or uint16 tensor, got %s" % x.dtype)
    if out_dtype not in _CONVERT_DTYPES:
        raise ValueError("resample(out_dtype=...) takes torch.float32, torch.float16 or torch.bfloat16, got %r" % (out_dtype,))
    if out_memory_format not in (torch.contiguous_format, torch.channels_last):
        raise ValueError("resample(out_memory_format=...) takes torch.contiguous_format or torch.channels_last, got %r" % (out_memory_format,))
    if x.dim() not in (2, 3, 4):
        raise ValueError("resample() takes a tensor of shape (H, W), (B, H, W) or (B, C, H, W)")
    nhwc_out = out_memory_format == torch.channels_last
    if nhwc_out and x.dim() != 4:
        raise ValueError("resample(out_memory_format=torch.channels_last) takes a tensor of shape (B, C, H, W)")
    if x.dim() == 4 and x.shape[1] > 4:
        raise ValueError("resample(integer=True) takes at most 4 channels, got %d" % x.shape[1])
    C = x.shape[1] if x.dim() == 4 else 1
    convert = api.make_convert(max(C, 1), _CONVERT_DTYPES[out_dtype], False, scale, offset)      # (checks the lengths of scale and offset)
    if not x.is_cuda:
        raise ValueError("resample() takes a tensor on a GPU (the library has no CPU path)")
    H, W = x.shape[-2], x.shape[-1]
    rq, lay = _query(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    iso = (lay.dst_iso_x, lay.dst_iso_y)
    dH, dW = lay.dst_height, lay.dst_width
    lead = tuple(x.shape[:-2])
    x = x.detach()
    y = torch.empty(lead + (dH, dW), dtype=out_dtype, device=x.device, **({"memory_format": torch.channels_last} if nhwc_out else {}))
    if 0 in lead or dH == 0 or dW == 0:
        return y, iso
    src_dtype, stream = _INT_DTYPES[x.dtype], None
    # (B, C, H, W) with C > 1: dense in channels_last the NHWC storage is the library's interleaved layout and is read in place; a
    # contiguous one that goes to a contiguous y runs plane by plane, also in place; a contiguous one that goes to channels_last is
    # brought into channels_last first (a copy of the integer tensor: the one case that copies)
    interleaved = C > 1 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    if C > 1 and not interleaved and nhwc_out:
        x = x.contiguous(memory_format=torch.channels_last)
        interleaved = True
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream().cuda_stream
        if interleaved:
            B = x.shape[0]
            _ensure_prepared(rq, C)
            convert.out_layout = L.LAYOUT_INTERLEAVED if nhwc_out else L.LAYOUT_PLANAR
            api.resample_convert_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C if nhwc_out else dW, src_dtype, convert, stream=stream, batch=B,
                                        src_image_stride=H * W * C, dst_image_stride=dH * dW * C, dst_plane_stride=dH * dW)
        else:
            # single-channel images: every image of a (H, W) / (B, H, W) tensor at once, or plane c of every image of a contiguous
            # (B, C, H, W) tensor with its channel's scale and offset
            x = x.contiguous()
            _ensure_prepared(rq, 1)
            images = x.numel() // max(H * W * C, 1)
            for c in range(C):
                one = api.make_convert(1, _CONVERT_DTYPES[out_dtype], False, convert.scale[c], convert.offset[c])
                api.resample_convert_device(rq, 1, x.data_ptr() + c * H * W * x.element_size(), W, y.data_ptr() + c * dH * dW * y.element_size(), dW, src_dtype, one,
                                            stream=stream, batch=images, src_image_stride=H * W * C, dst_image_stride=dH * dW * C)
    return y, iso


class _ResampleInterleaved(torch.autograd.Function):
    """(B, C, H, W) dense in torch.channels_last, 2 <= C <= 4: the NHWC storage is the library's interleaved layout, nothing is copied"""

    @staticmethod
    def forward(ctx, x, rq, lay, planned=False):
        """planned: False (the general interleaved adjoint), "any" (aai_adjoint_rotated_interleaved_device_f32) or "separable"
        (aai_adjoint_planned_interleaved_device_f32 at a geometry the separable kernel serves); _SAMPLER: a bilinear / bicubic request,
        aai_adjoint_sample_interleaved_device_f32"""
        B, C, H, W = x.shape
        dH, dW = lay.dst_height, lay.dst_width
        y = torch.empty((B, C, dH, dW), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        ctx.rq, ctx.src_shape, ctx.planned = rq, (B, C, H, W), planned
        with torch.cuda.device(x.device):
            _ensure_prepared(rq, C)
            if planned and planned != _SAMPLER and ctx.needs_input_grad[0]:
                _ensure_adjoint_prepared(rq, "separable" if planned == "separable" else "interleaved")
            api.resample_interleaved_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), dW * C, stream=torch.cuda.current_stream().cuda_stream,
                                            batch=B, src_image_stride=H * W * C, dst_image_stride=dH * dW * C)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return _adjoint_interleaved_f32(ctx.rq, ctx.src_shape, ctx.planned, gy), None, None, None


def _adjoint_interleaved_f32(rq, src_shape, planned, gy):
    """gx (fp32, (B, C, H, W) channels_last) = W^T gy for a (B, C, dH, dW) gradient of any float dtype and layout: the backward of
    _ResampleInterleaved and, widened, of _ResampleHalfInterleaved"""
    B, C, H, W = src_shape
    if gy.dtype != torch.float32:
        gy = gy.float()
    gy = gy.contiguous(memory_format=torch.channels_last)
    gx = torch.empty((B, C, H, W), dtype=torch.float32, device=gy.device, memory_format=torch.channels_last)
    dH, dW = gy.shape[2], gy.shape[3]
    with torch.cuda.device(gy.device):
        if planned == _SAMPLER:
            api.adjoint_sample_interleaved_device(rq, C, gy.data_ptr(), dW * C, gx.data_ptr(), W * C, stream=torch.cuda.current_stream().cuda_stream,
                                                  batch=B, dst_image_stride=dH * dW * C, src_image_stride=H * W * C)
        else:
            api.adjoint_interleaved_device(rq, C, gy.data_ptr(), dW * C, gx.data_ptr(), W * C, stream=torch.cuda.current_stream().cuda_stream,
                                           batch=B, dst_image_stride=dH * dW * C, src_image_stride=H * W * C, planned=planned)
    return gx


class _ResampleF64(torch.autograd.Function):
    """y = W x on a contiguous float64 (B, H, W) tensor: aai_resample_batch_device_f64.  No plan, nothing to prepare.  Its backward is
    _AdjointF64, whose backward is this function again: W is linear, so the pair differentiates to any order."""

    @staticmethod
    def forward(ctx, x, rq, lay):
        B, H, W = x.shape
        x = x.contiguous()
        y = torch.empty((B, lay.dst_height, lay.dst_width), dtype=torch.float64, device=x.device)
        ctx.rq, ctx.lay = rq, lay
        if B:
            with torch.cuda.device(x.device):
                api.resample_device_f64(rq, x.data_ptr(), W, y.data_ptr(), lay.dst_width, stream=torch.cuda.current_stream().cuda_stream,
                                        batch=B, src_image_stride=H * W, dst_image_stride=lay.dst_height * lay.dst_width)
        return y

    @staticmethod
    def backward(ctx, gy):
        return _AdjointF64.apply(gy, ctx.rq, ctx.lay), None, None


class _AdjointF64(torch.autograd.Function):
    """gx = W^T gy on a float64 (B, dH, dW) tensor: aai_adjoint_batch_device_f64; its backward is _ResampleF64"""

    @staticmethod
    def forward(ctx, gy, rq, lay):
        B, dH, dW = gy.shape
        H, W = rq.src_height, rq.src_width
        gy = gy.contiguous()
        gx = torch.empty((B, H, W), dtype=torch.float64, device=gy.device)
        ctx.rq, ctx.lay = rq, lay
        if B:
            with torch.cuda.device(gy.device):
                api.adjoint_device_f64(rq, gy.data_ptr(), dW, gx.data_ptr(), W, stream=torch.cuda.current_stream().cuda_stream,
                                       batch=B, dst_image_stride=dH * dW, src_image_stride=H * W)
        return gx

    @staticmethod
    def backward(ctx, ggx):
        return _ResampleF64.apply(ggx, ctx.rq, ctx.lay), None, None


def _resample_f64(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy):
    """resample(..., f64=True): the reference-precision operator on a float64 tensor (include/aai_f64.h)"""
    if x.dtype != torch.float64:
        raise TypeError("resample(f64=True) takes a float64 tensor, got %s" % x.dtype)
    if x.dim() not in (2, 3, 4):
        raise ValueError("resample() takes a tensor of shape (H, W), (B, H, W) or (B, C, H, W)")
    if not x.is_cuda:
        raise ValueError("resample() takes a tensor on a GPU (the library has no CPU path)")
    if mode not in (L.MODE_AREA, L.MODE_FAST):
        raise ValueError("resample(f64=True): the area and fast modes only (the bilinear / bicubic comparison paths have no float64 path)")
    H, W = x.shape[-2], x.shape[-1]
    rq, lay = _query(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    iso = (lay.dst_iso_x, lay.dst_iso_y)
    lead = tuple(x.shape[:-2])
    if 0 in lead:
        return torch.empty(lead + (lay.dst_height, lay.dst_width), dtype=torch.float64, device=x.device), iso
    # every rank through the (B, H, W) operator; a 4-D tensor plane by plane (channels_last and other strided input is made contiguous)
    y = _ResampleF64.apply(x.contiguous().view(-1, H, W), rq, lay)
    return y.view(lead + (lay.dst_height, lay.dst_width)), iso


_NO_SAMPLER_ADJOINT = ("resample(): the bilinear / bicubic comparison paths have no adjoint; detach x or run under torch.no_grad() "
                       "(or pass sampler_backward=True for the samplers' own adjoint)")


def _query(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy):
    rq = api.make_request(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    rc, msg, lay = api.query(rq)
    if rc != L.OK:
        raise api.AaiError(rc, msg)
    return rq, lay


def _resample_nchw(x, geometry, mode, policy, planned, sampler_backward=False):
    B, C, H, W = x.shape
    rq, lay = _query(W, H, *geometry, mode, policy)
    iso = (lay.dst_iso_x, lay.dst_iso_y)
    if B == 0 or C == 0:
        return torch.empty((B, C, lay.dst_height, lay.dst_width), dtype=torch.float32, device=x.device), iso
    if x.requires_grad and torch.is_grad_enabled() and mode not in (L.MODE_AREA, L.MODE_FAST) and not sampler_backward:
        raise ValueError(_NO_SAMPLER_ADJOINT)
    interleaved = 2 <= C <= 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    interleaved, planned = _nchw_route(interleaved, lay, mode, planned, sampler_backward)
    if interleaved:
        return _ResampleInterleaved.apply(x, rq, lay, planned), iso
    y = _Resample.apply(x.contiguous().view(B * C, H, W), rq, lay, planned)
    return y.view(B, C, lay.dst_height, lay.dst_width), iso


def _nchw_route(interleaved, lay, mode, planned, sampler_backward):
    """The route of a (B, C, H, W) fp32 tensor and of its backward (the table in resample()'s docstring).  interleaved: whether the tensor
    is dense in channels_last with 2 <= C <= 4.  -> (the interleaved route?, `planned` as _ResampleInterleaved / _Resample take it)"""
    if mode not in (L.MODE_AREA, L.MODE_FAST) and sampler_backward:
        # the samplers' adjoint: the route is the forward's (planned_backward chooses between adjoints of the area / fast modes only)
        return interleaved, _SAMPLER
    if planned == "channels_last":
        if interleaved and lay.kernel == L.KERNEL_AXIS:
            return True, "separable"     # zero-copy AND the transposed separable backward
        planned = "interleaved"      # every other input: exactly "interleaved"
    if planned == "interleaved":
        if interleaved and lay.kernel in (L.KERNEL_ROTATED, L.KERNEL_FAST):
            return True, "any"           # zero-copy AND the planned backward
        planned = "any"              # every other input: exactly "any"
    if interleaved and planned and lay.kernel == L.KERNEL_AXIS:
        interleaved = False          # the planned adjoint is single-channel, and far faster there than the interleaved gather
    if interleaved and planned == "any" and lay.kernel in (L.KERNEL_ROTATED, L.KERNEL_FAST):
        interleaved = False          # ... and so is the planned adjoint at general rotations
    return interleaved, (False if interleaved else planned)


def resample(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE,
             *positional, sampler_backward=False, f64=False, half=False, integer=False, half_backward=False,
             out_dtype=None, scale=None, offset=None, out_memory_format=torch.contiguous_format, planned_backward=False):
    """Resample a CUDA/HIP fp32 tensor of shape (H, W), (B, H, W) or (B, C, H, W); returns ``(y, dst_isocenter)`` with y of shape
    (dH, dW), (B, dH, dW) or (B, C, dH, dW).  Differentiable ONCE with respect to x in the area and fast modes (a double backward raises; the
    bilinear / bicubic comparison paths are differentiable only with sampler_backward=True, below: without it an x that requires grad
    raises ValueError there).  Non-contiguous
    input is made contiguous; other dtypes raise TypeError, CPU tensors and other ranks ValueError, an invalid geometry
    AaiError.

    planned_backward: False (the default) -- the backward is aai_adjoint_batch_device_f32, the double-precision gather at every
    rotation.  True -- the backward is aai_adjoint_planned_batch_device_f32: at rotations by multiples of 90 degrees the transposed
    separable kernel on the forward's own plan (fp32 weights and sums, within a few 1e-7 relative of the default, and one to two
    orders of magnitude faster there), the default's kernels and bits at every other rotation.  With True and an x that requires
    grad the forward also builds the plan's adjoint tables (aai_adjoint_prepare; it synchronises once per geometry and device), so
    inside a stream capture a geometry without them raises RuntimeError, like a geometry without a plan.  "any" -- the backward is
    aai_adjoint_rotated_batch_device_f32: exactly True at multiples of 90 degrees; at every other rotation the default's BITS from the
    plan's cached sums (8 bytes per dst pixel on the device) and the plain closed forms, and with an x that requires grad the forward
    builds those tables (aai_adjoint_rotated_prepare; the same rule inside a stream capture).  "interleaved" -- exactly "any" for
    every input but one: a (B, C, H, W) tensor dense in torch.channels_last with 2 <= C <= 4 at a geometry the rotated area / fast
    kernels serve keeps the zero-copy interleaved route AND gets a planned backward, aai_adjoint_rotated_interleaved_device_f32 (the
    same tables, on the single-channel plan, built by the forward when x requires grad; the same rule inside a stream capture).  Any
    "channels_last" -- exactly "interleaved" for every input but one: such a channels_last tensor at a geometry the SEPARABLE kernel
    serves (aai_query: AAI_KERNEL_AXIS, rotations by multiples of 90 degrees) keeps the zero-copy interleaved route too, and its backward
    is aai_adjoint_planned_interleaved_device_f32, the interleaved transposed separable kernel (the tables of True, on the single-channel
    plan, built by the forward through aai_adjoint_rotated_prepare when x requires grad; the same rule inside a stream capture).  Any
    other string raises ValueError.

    (B, C, H, W) input takes one of two routes, every plane resampled with the same geometry.  Which one, by planned_backward
    (cl = dense in channels_last with 2 <= C <= 4; "other" = bilinear / bicubic):
      geometry served by      False              True               "any"              "interleaved"                   "channels_last"
      separable kernel, cl    interleaved        planar             planar             planar                          interleaved, separable backward
      rotated / fast, cl      interleaved        interleaved        planar             interleaved, planned backward   interleaved, planned backward
      other, cl               interleaved        interleaved        interleaved        interleaved                     interleaved
      any, not cl             planar             planar             planar             planar                          planar
      planar       x.contiguous() viewed as (B * C, H, W) through the 3-D operator and reshaped back: the 3-D operator's bits plane by
                   plane, planned_backward honoured.  Every input the interleaved route does not take, channels_last tensors with
                   C = 1 or C > 4 among them.
      interleaved  x dense in torch.channels_last (and not dense in the default format) with 2 <= C <= 4: zero-copy on the NHWC
                   storage.  Forward aai_resample_interleaved_device (the plan prepared for C channels; y is channels_last and within
                   the library's tolerance of the planar forward, not its bits); backward aai_adjoint_interleaved_device_f32 on a
                   channels_last gy (x.grad is channels_last; each channel has the bits of the default single-channel adjoint, a
                   pair's weight computed once for all channels).
                   EXCEPTION: with planned_backward=True and a geometry the separable kernel serves (aai_query: AAI_KERNEL_AXIS)
                   the planar route is taken -- the planned adjoint is single-channel and one to two orders of magnitude faster
                   there than the general gather, which the interleaved adjoint is.  The same holds for planned_backward="any" at
                   every geometry its single-channel path serves (the separable kernel's, and the rotated area / fast kernels').
                   planned_backward="interleaved" lifts the second half of the exception: at a geometry the rotated area / fast
                   kernels serve the route stays interleaved and the backward is aai_adjoint_rotated_interleaved_device_f32 on a
                   channels_last gy -- y and x.grad are channels_last and have the bits of this route's default (y: the interleaved
                   forward's; x.grad: per channel the default single-channel adjoint's, which are also the "any" planar route's).
                   At the separable kernel's geometries "interleaved" stays planar.
                   planned_backward="channels_last" lifts the first half as well: at a geometry the separable kernel serves the route
                   stays interleaved and the backward is aai_adjoint_planned_interleaved_device_f32 on a channels_last gy
                   (aai_axis_adjoint_multi_kernel<C>, one lane per row element) -- y and x.grad are channels_last; y has the
                   interleaved forward's bits (within the library's tolerance of the planar forward), x.grad[b, c] the bits of the
                   planar planned_backward=True gradient.  A wide separable plan (AAI_KERNEL_AXIS_WIDE) is "other" in every column.
                   The rule for an exception was: a row class whose backward is not faster on this route than on the planar one
                   keeps the planar route.  Measured on an MI355X for C = 3 and 4 (profiles/adjoint_axis_interleaved_time.txt, one
                   run; DESIGN.md section 9 quotes it), the backward alone with the planar route's permutes included: this route's
                   median is below the planar route's in all 16 rows -- 1.5-2.0x when down-sampling, 2.8-4.5x at x2 up-sampling at 270
                   degrees (1.080 -> 0.384 ms for C = 3 in area mode) -- so there is no exception.
                   Measured on an MI355X for C = 3 and 4 (profiles/adjoint_rotated_interleaved_time.txt, one run; DESIGN.md section 9
                   quotes it): the new backward is 1.9-4.2x faster than the general interleaved backward and 2.5-3.5x faster than C
                   planned single-channel backwards on planes split beforehand (the planar route's permutes not counted), with
                   identical bits in every row.
    sampler_backward: False (the default) -- nothing changes: a bilinear / bicubic x that requires grad raises ValueError.  True -- such an
    x is accepted and the operator is differentiable ONCE there too: the backward is aai_adjoint_sample_batch_device_f32 on
    torch.cuda.current_stream(), gsrc = W^T gdst for the sampler's own W (the forward's affine map and quadrant pre-rotation,
    clamp-to-edge taps that add up, exact zeros outside the image extent, Keys a = -0.5) -- one deterministic gather per source
    pixel with double-precision weights, no plan, no scratch, nothing to prepare, capturable.  (B, C, H, W) input dense in
    channels_last with 2 <= C <= 4 keeps the zero-copy interleaved route and its backward is
    aai_adjoint_sample_interleaved_device_f32 (x.grad is channels_last, channel c with the bits of the single-channel entry on
    plane c); every other input takes the planar route.  planned_backward is not consulted there, and in the area / fast modes
    sampler_backward has no effect.

    f64: False (the default) -- nothing changes: a float64 tensor raises TypeError.  True -- the reference-precision operator
    (include/aai_f64.h): x must be a float64 tensor (float32 raises TypeError) on a GPU, of shape (H, W), (B, H, W) or (B, C, H, W); the area and
    fast modes only (a sampler mode raises ValueError, whether or not x requires grad).  The forward is aai_resample_batch_device_f64,
    the backward aai_adjoint_batch_device_f64, both on torch.cuda.current_stream(), no value ever rounded to fp32.  The two are
    autograd Functions that are each other's backward, so the operator differentiates to ANY order and torch.autograd.gradcheck /
    gradgradcheck pass.  There is no plan: nothing is prepared, the first call of a geometry only enqueues, and the call works inside
    a stream capture on a geometry never seen before.  A 4-D input always takes the planar route (channels_last and other strided input
    is made contiguous; y is contiguous).  planned_backward and sampler_backward are not consulted.

    half: False (the default) -- nothing changes: a float16 / bfloat16 tensor raises TypeError.  True -- the half-precision operator
    (include/aai_half.h): x must be a float16 or bfloat16 tensor (float32 raises TypeError) on a GPU, of shape (H, W), (B, H, W) or
    (B, C, H, W); y has x's dtype.  The forward is aai_resample_half_batch_device on torch.cuda.current_stream(): every element widened
    exactly, fp32 weights and sums, ONE rounding to x's dtype; rotations by 0 / 180 degrees in the area / fast modes run one streaming
    kernel on the half tensors, every other request widens into scratch, runs the fp32 forward and narrows.  The plan is the fp32
    forward's: the first call of a geometry prepares it, and inside a stream capture an unprepared geometry raises RuntimeError.  A 4-D
    input always takes the planar route (channels_last and other strided input is made contiguous; y is contiguous).  The area and fast
    modes are differentiable ONCE: the backward widens gy to fp32, runs the fp32 adjoint with planned_backward honoured as for an fp32
    tensor ("interleaved" and "channels_last" mean "any": there is no interleaved route), and rounds the gradient to x's dtype;
    bilinear / bicubic with sampler_backward=True likewise.  torch.autocast does not route here by itself.
    "channels_last" -- exactly True for every input but one: a float16 / bfloat16 (B, C, H, W) tensor dense in torch.channels_last (and not
    dense in the default format) with 2 <= C <= 4 is read IN PLACE as B interleaved images (include/aai_half_interleaved.h:
    aai_resample_half_interleaved_device on torch.cuda.current_stream(); the plan is the fp32 interleaved forward's for C channels) and
    y is channels_last in x's dtype: nothing is copied.  Per channel the values keep half=True's contract; the bits are the interleaved
    entry's (within one unit in the last place of the planar route's).  The backward widens gy to fp32 channels_last, runs the backward
    the table above gives an fp32 channels_last tensor under the same planned_backward -- "interleaved" and "channels_last" keep their
    meaning here, they do not collapse to "any" -- or, bilinear / bicubic with sampler_backward=True,
    aai_adjoint_sample_interleaved_device_f32, and rounds the gradient once to x's dtype; x.grad is channels_last.
      half=            channels_last tensor, 2 <= C <= 4        every other tensor
      True             made contiguous, planar, y contiguous    planar
      "channels_last"  in place, interleaved, y channels_last   exactly True
    Any other string raises ValueError.

    half_backward: False (the default) -- nothing changes.  True (keyword-only; needs half=True or half="channels_last", an area or fast
    mode and planned_backward left at False: anything else raises ValueError) -- the forward is half's, and the backward stays in x's
    dtype: gy, made dense in y's layout, goes straight to aai_adjoint_half_device (include/aai_adjoint_half.h) on
    torch.cuda.current_stream() and what that writes is x.grad -- no fp32 copy of gy, no fp32 gradient image, no conversion kernel.  At
    rotations by multiples of 90 degrees (plans without correction lists) that is ONE kernel on the half tensors; every other request --
    and one class that measured no faster that way, a single-channel image up-sampled at 90 / 270 degrees
    (profiles/adjoint_half_time.txt) -- widens into the library's scratch, runs the fp32 planned adjoint and narrows: the same bits.  Planar tensors of any rank go as B * C single-channel
    images and x.grad has the bits of half=True, planned_backward="any"; a channels_last tensor that half="channels_last" reads in place
    goes as B interleaved images, x.grad is channels_last and has the bits of half="channels_last", planned_backward="channels_last".  With
    an x that requires grad the forward builds the single-channel plan's adjoint tables (aai_adjoint_rotated_prepare; it synchronises once
    per geometry and device), so inside a stream capture a geometry without them raises RuntimeError.  Differentiable ONCE.

    integer: False (the default) -- nothing changes: a uint8 / uint16 tensor raises TypeError.  True -- the integer operator
    (include/aai_int.h): x must be a torch.uint8 tensor (or torch.uint16 where this torch has that dtype; float32 raises TypeError) on a
    GPU, of shape (H, W), (B, H, W) or (B, C, H, W) with C <= 4; y has x's dtype.  The forward is aai_resample_int_batch_device on
    torch.cuda.current_stream(): every element as its integer value, fp32 weights and sums, ONE conversion -- round to nearest, ties to
    even, saturate to the range of the dtype; rotations by 0 / 180 degrees in the area / fast modes run one streaming kernel on the
    integer tensors, every other request runs the fp32 forward into scratch and converts.  A (B, C, H, W) tensor dense in
    torch.channels_last is read in place as B interleaved images and y is channels_last; a contiguous one with C > 1 runs as B * C
    single-channel images (other strided input is made contiguous).  The plan is the fp32 forward's for that channel count: the first
    call of a geometry prepares it, and inside a stream capture an unprepared geometry raises RuntimeError.  There is no autograd
    (integers carry no gradient): y never requires grad.  integer=True together with half, f64, planned_backward or sampler_backward
    raises ValueError.

    out_dtype: None (the default) -- nothing changes.  torch.float32, torch.float16 or torch.bfloat16, with integer=True (without it:
    ValueError) -- resample and convert (include/ext/aai_convert.h): x is a uint8 / uint16 tensor exactly as integer=True takes it, y is a
    tensor of out_dtype holding round(fma(s, scale[c], offset[c])): the fp32 sums s of the integer values, ONE fused multiply-add in fp32,
    ONE rounding to out_dtype (to nearest, ties to even; beyond the largest finite float16: +-Inf).  scale / offset: a scalar or one value
    per channel (defaults 1 and 0; finite).  out_memory_format: torch.contiguous_format (y is planar, NCHW) or torch.channels_last (y has
    NHWC storage; (B, C, H, W) tensors only); the library writes y in that format, nothing is permuted or cast afterwards.  A (B, C, H, W)
    x dense in channels_last is read in place; a contiguous one going to a contiguous y runs plane by plane in place; a contiguous one
    going to channels_last is copied into channels_last first.  Rotations by 0 / 180 degrees in the area / fast modes run one kernel from
    the integer tensor to y, every other request runs the fp32 forward into scratch and converts.  y never requires grad.  out_dtype
    together with half, f64, planned_backward, sampler_backward or half_backward raises ValueError; scale, offset or a channels_last
    out_memory_format without out_dtype raise ValueError.

    B == 0 or C == 0 returns an empty tensor of the output's shape without a launch."""
    # planned_backward keeps its place as the eighth positional argument (*positional holds at most that one); sampler_backward is
    # keyword-only
    if positional:
        if len(positional) > 1 or planned_backward is not False:
            raise TypeError("resample() takes at most 8 positional arguments, planned_backward the last of them, and planned_backward only once")
        planned_backward = positional[0]
    if not isinstance(x, torch.Tensor):
        raise TypeError("resample() takes a torch.Tensor")
    if out_dtype is not None:
        if not integer:
            raise ValueError("resample(out_dtype=...) converts integer tensors: it needs integer=True")
        if half or f64 or planned_backward is not False or sampler_backward or half_backward:
            raise ValueError("resample(integer=True, out_dtype=...) has no gradient: it takes none of half, f64, planned_backward, sampler_backward, half_backward")
        return _resample_convert(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy, out_dtype, scale, offset, out_memory_format)
    if scale is not None or offset is not None or out_memory_format != torch.contiguous_format:
        raise ValueError("resample(): scale, offset and out_memory_format belong to out_dtype (with integer=True)")
    if isinstance(half, str) and half != "channels_last":
        raise ValueError('half must be False, True or "channels_last", got %r' % (half,))
    if half_backward:
        if not half:
            raise ValueError('resample(half_backward=True) needs half=True or half="channels_last": it is the backward of the half-precision operator')
        if planned_backward is not False:
            raise ValueError("resample(half_backward=True) names its backward itself: planned_backward must stay False, got %r" % (planned_backward,))
        if mode not in (L.MODE_AREA, L.MODE_FAST):
            raise ValueError("resample(half_backward=True): the area and fast modes only (the samplers' adjoint has no half-precision entry)")
    if integer:
        if half or f64 or planned_backward is not False or sampler_backward:
            raise ValueError("resample(integer=True) has no gradient and one element type: it takes none of half, f64, planned_backward, sampler_backward")
        return _resample_int(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    if f64:
        return _resample_f64(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    if half:
        return _resample_half(x, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy, _normalise_planned(planned_backward),
                              bool(sampler_backward), channels_last=half == "channels_last", half_backward=bool(half_backward))
    if x.dtype != torch.float32:
        raise TypeError("resample() takes a float32 tensor, got %s" % x.dtype)
    if x.dim() not in (2, 3, 4):
        raise ValueError("resample() takes a tensor of shape (H, W), (B, H, W) or (B, C, H, W)")
    if not x.is_cuda:
        raise ValueError("resample() takes a tensor on a GPU (the library has no CPU path)")
    if x.dim() == 4:
        return _resample_nchw(x, (src_resolution, dst_resolution, src_isocenter, rotation_angle), mode, policy, _normalise_planned(planned_backward),
                              bool(sampler_backward))
    xb = (x if x.dim() == 3 else x.unsqueeze(0)).contiguous()
    rq = api.make_request(xb.shape[2], xb.shape[1], src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    rc, msg, lay = api.query(rq)
    if rc != L.OK:
        raise api.AaiError(rc, msg)
    if xb.requires_grad and torch.is_grad_enabled() and mode not in (L.MODE_AREA, L.MODE_FAST) and not sampler_backward:
        raise ValueError(_NO_SAMPLER_ADJOINT)
    planned = _normalise_planned(planned_backward)
    if planned in ("interleaved", "channels_last"):
        planned = "any"              # there are no channels to interleave
    if sampler_backward and mode not in (L.MODE_AREA, L.MODE_FAST):
        planned = _SAMPLER           # (planned_backward chooses between adjoints of the area / fast modes only)
    y = _Resample.apply(xb, rq, lay, planned)
    return (y if x.dim() == 3 else y.squeeze(0)), (lay.dst_iso_x, lay.dst_iso_y)
