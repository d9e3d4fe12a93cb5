"""ctypes loader for libaai_hip.so (the C ABI declared in include/aai.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C area_average_interpolation_amd/csrc``.
There is no Python or CPU fallback: if the shared object is missing, importing the compute API raises.
"""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# (AAI_LIB points the loader at another build of the library, e.g. `make -C csrc OUT=... OBJ=...`, to compare two builds)
LIB_PATH = os.environ.get("AAI_LIB") or os.path.join(_HERE, "libaai_hip.so")

# status codes (include/aai.h)
OK = 0
ERR_RESOLUTION_MISMATCH = 1
ERR_RESOLUTION_NONPOSITIVE = 2
ERR_NO_ROWS = 3
ERR_NO_COLUMNS = 4
ERR_NONFINITE = 5
ERR_BAD_ARGUMENT = 6
ERR_TOO_LARGE = 7
ERR_NO_DEVICE = 8
ERR_HIP = 9
ERR_EMPTY_OUTPUT = 10

MODE_AREA, MODE_FAST, MODE_BILINEAR, MODE_BICUBIC = 1, 2, 3, 4
POLICY_REFERENCE, POLICY_EXACT = 0, 1
POLICY_DOUBLE_PRECISION = 0x100      # OR into a policy: general rotations in double precision throughout (include/aai.h)
POLICY_PREFER_CELL = 0x200           # OR into a policy: the cell formulation also for small outputs (a hint)
POLICY_DIAG_NO_FIXUP = 0x400         # OR into a policy: DIAGNOSTIC, the fix-up pass over the plan's listed pixels is not launched
DTYPE_F32, DTYPE_U8, DTYPE_U16 = 0, 1, 2
HALF_F16, HALF_BF16 = 1, 2           # include/aai_half.h: AAI_HALF_F16 / AAI_HALF_BF16, IEEE binary16 / bfloat16 as raw 16-bit elements
KERNEL_AXIS, KERNEL_ROTATED, KERNEL_FAST, KERNEL_SAMPLE, KERNEL_AXIS_WIDE = 1, 2, 3, 4, 5


class Request(ctypes.Structure):
    """struct aai_request"""
    _fields_ = [("mode", ctypes.c_int32), ("policy", ctypes.c_int32),
                ("src_width", ctypes.c_int32), ("src_height", ctypes.c_int32),
                ("src_res_x", ctypes.c_double), ("src_res_y", ctypes.c_double),
                ("dst_res_x", ctypes.c_double), ("dst_res_y", ctypes.c_double),
                ("src_iso_x", ctypes.c_double), ("src_iso_y", ctypes.c_double),
                ("rotation_deg", ctypes.c_double)]


class Layout(ctypes.Structure):
    """struct aai_layout"""
    _fields_ = [("dst_width", ctypes.c_int32), ("dst_height", ctypes.c_int32),
                ("dst_iso_x", ctypes.c_double), ("dst_iso_y", ctypes.c_double),
                ("scale", ctypes.c_int32), ("quadrant", ctypes.c_int32),
                ("reduced_angle_deg", ctypes.c_double), ("side", ctypes.c_double),
                ("kernel", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# every symbol include/aai.h declares: name -> (restype, argtypes)
_P = ctypes.c_void_p
_RQ = ctypes.POINTER(Request)
_LY = ctypes.POINTER(Layout)
_I64 = ctypes.c_int64
SYMBOLS = {
    "aai_query": (ctypes.c_int, [_RQ, _LY]),
    "aai_last_error": (ctypes.c_char_p, []),
    "aai_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "aai_version": (ctypes.c_int, []),
    "aai_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "aai_set_device": (ctypes.c_int, [ctypes.c_int]),
    "aai_device_synchronize": (ctypes.c_int, []),
    "aai_resample_f32": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
    "aai_resample_f64": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
    "aai_resample_device_f32": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _P]),
    "aai_resample_batch_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_resample_batch_multi_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                          ctypes.POINTER(_P), _I64, _I64, ctypes.POINTER(_P), _I64, _I64, ctypes.POINTER(_P)]),
    "aai_resample_batch_device": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, ctypes.c_int32, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_resample_host": (ctypes.c_int, [_RQ, _P, ctypes.c_int32, _I64, _P, _I64, _LY]),
    "aai_resample_interleaved_device": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int32, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_resample_interleaved_host": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, ctypes.c_int32, _I64, _P, _I64, _LY]),
    "aai_host_alloc": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64]),
    "aai_host_free": (ctypes.c_int, [_P]),
    "aai_resample_batch_host": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, ctypes.c_int32, _I64, _I64, _P, _I64, _I64, _LY]),
    "aai_band_source_rows": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "aai_resample_band_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _P, _I64, _P]),
    "aai_adjoint_batch_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_f32": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
    "aai_synth_device_f32": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _I64, ctypes.c_uint64, _P]),
    "aai_synth_rows_device_f32": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _I64, ctypes.c_uint64, _P]),
    "aai_prepare": (ctypes.c_int, [_RQ, ctypes.c_int32]),
    "aai_plan_info": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]),
    "aai_shutdown": (ctypes.c_int, []),
    "aai_last_kernel": (ctypes.c_char_p, []),
}
# the extension header include/aai_adjoint_planned.h (SYMBOLS mirrors include/aai.h, entry for entry)
PLANNED_SYMBOLS = {
    "aai_adjoint_prepare": (ctypes.c_int, [_RQ]),
    "aai_adjoint_planned_batch_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_planned_f32": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_adjoint_interleaved.h
INTERLEAVED_ADJOINT_SYMBOLS = {
    "aai_adjoint_interleaved_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_interleaved_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_adjoint_rotated.h
ROTATED_ADJOINT_SYMBOLS = {
    "aai_adjoint_rotated_prepare": (ctypes.c_int, [_RQ]),
    "aai_adjoint_rotated_batch_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_rotated_f32": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_adjoint_rotated_interleaved.h
ROTATED_INTERLEAVED_ADJOINT_SYMBOLS = {
    "aai_adjoint_rotated_interleaved_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_rotated_interleaved_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_adjoint_planned_interleaved.h
PLANNED_INTERLEAVED_ADJOINT_SYMBOLS = {
    "aai_adjoint_planned_interleaved_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_planned_interleaved_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_adjoint_sample.h: the adjoint of the bilinear / bicubic samplers (the argument lists of
# aai_adjoint_batch_device_f32, aai_adjoint_f32, aai_adjoint_interleaved_device_f32, aai_adjoint_interleaved_f32)
SAMPLE_ADJOINT_SYMBOLS = {
    "aai_adjoint_sample_batch_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_sample_f32": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
    "aai_adjoint_sample_interleaved_device_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_sample_interleaved_f32": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_f64.h: the reference-precision path, double images end to end (the argument lists of
# aai_resample_batch_device_f32, aai_resample_f64, aai_adjoint_batch_device_f32, aai_adjoint_f32)
F64_SYMBOLS = {
    "aai_resample_batch_device_f64": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_resample_exact_f64": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
    "aai_adjoint_batch_device_f64": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_f64": (ctypes.c_int, [_RQ, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_half.h: fp16 / bf16 images in and out (aai_resample_batch_device_f32's argument list with the element
# type behind the batch; aai_resample_f32's with it behind the request)
HALF_SYMBOLS = {
    "aai_resample_half_batch_device": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_resample_half_host": (ctypes.c_int, [_RQ, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_int.h: u8 / u16 images in and out (aai_resample_interleaved_device's argument list with the element
# type behind the channels; aai_resample_interleaved_host's likewise)
INT_SYMBOLS = {
    "aai_resample_int_batch_device": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_resample_int_host": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_half_interleaved.h: fp16 / bf16 images of 1..4 interleaved channels in and out (the argument lists of
# include/aai_int.h's entries, the half element type in the place of the integer one)
HALF_INTERLEAVED_SYMBOLS = {
    "aai_resample_half_interleaved_device": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_resample_half_interleaved_host": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/aai_adjoint_half.h: the adjoint on fp16 / bf16 gradients of 1..4 interleaved channels (the argument lists of
# include/aai_adjoint_planned_interleaved.h's entries, the half element type behind the channels)
ADJOINT_HALF_SYMBOLS = {
    "aai_adjoint_half_device": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _P, _I64, _I64, _P]),
    "aai_adjoint_half_host": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _P, _I64, _LY]),
}

# the extension header include/ext/aai_convert.h: u8 / u16 images in, a scaled fp32 / fp16 / bf16 image out, interleaved or planar
LAYOUT_INTERLEAVED, LAYOUT_PLANAR = 0, 1


class Convert(ctypes.Structure):
    """aai_convert: out_type (DTYPE_F32, HALF_F16 or HALF_BF16), out_layout (LAYOUT_*), scale and offset per channel"""
    _fields_ = [("out_type", ctypes.c_int32), ("out_layout", ctypes.c_int32), ("scale", ctypes.c_float * 4), ("offset", ctypes.c_float * 4)]


_CV = ctypes.POINTER(Convert)
CONVERT_SYMBOLS = {
    "aai_resample_convert_device": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _CV, _P, _I64, _I64, _I64, _P]),
    "aai_resample_convert_host": (ctypes.c_int, [_RQ, ctypes.c_int32, ctypes.c_int32, _P, _I64, _CV, _P, _I64, _I64, _LY]),
}

_lib = None


def load():
    """Load libaai_hip.so, failing loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libaai_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the resampling path)" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64, and a process that loads the system's copy
        # first (through this library) and torch's afterwards finds "No HIP GPUs" in torch.  Loaded after torch, this
        # library binds to the copy already in the process (same SONAME) -- so bring torch in first when it is installed.
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SYMBOLS.items()) + list(PLANNED_SYMBOLS.items()) + list(INTERLEAVED_ADJOINT_SYMBOLS.items()) +
                                  list(ROTATED_ADJOINT_SYMBOLS.items()) + list(ROTATED_INTERLEAVED_ADJOINT_SYMBOLS.items()) +
                                  list(PLANNED_INTERLEAVED_ADJOINT_SYMBOLS.items()) + list(SAMPLE_ADJOINT_SYMBOLS.items()) + list(F64_SYMBOLS.items()) +
                                  list(HALF_SYMBOLS.items()) + list(INT_SYMBOLS.items()) + list(HALF_INTERLEAVED_SYMBOLS.items()) + list(ADJOINT_HALF_SYMBOLS.items()) +
                                  list(CONVERT_SYMBOLS.items())):
            fn = getattr(lib, name)      # AttributeError if the ABI and the header drifted apart
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
