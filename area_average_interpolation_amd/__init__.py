"""MI355X-native area-average image interpolation: Python plumbing over the C ABI in include/aai.h."""
from . import _lib
from ._lib import (DTYPE_F32, DTYPE_U8, DTYPE_U16, MODE_AREA, MODE_FAST, MODE_BILINEAR, MODE_BICUBIC, POLICY_REFERENCE, POLICY_EXACT, POLICY_DOUBLE_PRECISION,
                   HALF_F16, HALF_BF16, LAYOUT_INTERLEAVED, LAYOUT_PLANAR, Request, Layout, Convert)
from .api import (AreaAverageInterpolation, AaiError, PinnedArray, make_request, query, resample_host, resample_batch_host, precision_check, resample_interleaved_host, resample_interleaved_device, resample_device, resample_multi_device, adjoint_device, adjoint_host, adjoint_prepare, adjoint_rotated_prepare, adjoint_interleaved_device, adjoint_interleaved_host,
                  adjoint_sample_device, adjoint_sample_host, adjoint_sample_interleaved_device, adjoint_sample_interleaved_host,
                  resample_device_f64, adjoint_device_f64, resample_exact_host, adjoint_exact_host,
                  resample_half_device, resample_half_host, resample_half_interleaved_device, resample_half_interleaved_host, resample_int_device, resample_int_host,
                  make_convert, resample_convert_device, resample_convert_host,
                  adjoint_half_device, adjoint_half_host,
                  band_source_rows, resample_band_device, synth_device, synth_rows_device, prepare, plan_shape, shutdown, debug_cell_min_waves, debug_skip_fixup, device_count, set_device, synchronize, last_kernel, last_error)

__all__ = ["AreaAverageInterpolation", "AaiError", "PinnedArray", "make_request", "query", "resample_host", "resample_batch_host", "precision_check", "resample_interleaved_host", "resample_interleaved_device", "resample_device", "resample_multi_device", "adjoint_device", "adjoint_host", "adjoint_prepare", "adjoint_rotated_prepare", "adjoint_interleaved_device", "adjoint_interleaved_host", "resample",
           "adjoint_sample_device", "adjoint_sample_host", "adjoint_sample_interleaved_device", "adjoint_sample_interleaved_host",
           "resample_device_f64", "adjoint_device_f64", "resample_exact_host", "adjoint_exact_host",
           "resample_half_device", "resample_half_host", "HALF_F16", "HALF_BF16", "resample_half_interleaved_device", "resample_half_interleaved_host", "resample_int_device", "resample_int_host",
           "make_convert", "resample_convert_device", "resample_convert_host", "Convert", "LAYOUT_INTERLEAVED", "LAYOUT_PLANAR",
           "adjoint_half_device", "adjoint_half_host",
           "band_source_rows", "resample_band_device", "synth_device", "synth_rows_device", "prepare", "plan_shape", "shutdown", "debug_cell_min_waves", "debug_skip_fixup", "device_count", "set_device", "synchronize", "last_kernel", "last_error",
           "MODE_AREA", "MODE_FAST", "MODE_BILINEAR", "MODE_BICUBIC", "POLICY_REFERENCE", "POLICY_EXACT", "POLICY_DOUBLE_PRECISION",
           "Request", "Layout", "DTYPE_F32", "DTYPE_U8", "DTYPE_U16"]


def resample(*args, **kwargs):
    """torch_ops.resample: the differentiable torch operator (torch is imported on the first call, not with the package)"""
    from .torch_ops import resample as _resample
    return _resample(*args, **kwargs)
