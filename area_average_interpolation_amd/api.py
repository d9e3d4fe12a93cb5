"""Host-side mirror of the reference's call surface on top of the C ABI (libaai_hip.so).

The reference boundary is ``class AreaAverageInterpolation`` with two methods of identical signature
(/root/reference/Source.cpp:55-57 and 584-586)::

    pair<bool,string> areaAverageInterpolation    (IMG src, IMG &dst, dP srcResolution, dP dstResolution,
    pair<bool,string> fastAreaAverageInterpolation              dP srcIsocenter, dP &dstIsocenter, double rotationAngle)

Python has no out-parameters, so the two methods below keep the names, the argument order and meaning and
the error behaviour, and return ``((ok, message), dst, dstIsocenter)``; on failure ``dst`` and
``dstIsocenter`` are ``None`` (the reference leaves them untouched).  The C++ drop-in with the exact
reference signature is include/AreaAverageInterpolation.hpp.

Everything here is plumbing around the C ABI; all arithmetic happens in the HIP kernels.
"""
import ctypes

import numpy as np

from . import _lib as L


class AaiError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("aai error %d: %s" % (code, message))
        self.code, self.message = code, message


def _pair(v):
    if np.isscalar(v):
        return float(v), float(v)
    return float(v[0]), float(v[1])


def make_request(width, height, src_resolution, dst_resolution, src_isocenter, rotation_angle,
                 mode=L.MODE_AREA, policy=L.POLICY_REFERENCE):
    sr, dr, iso = _pair(src_resolution), _pair(dst_resolution), _pair(src_isocenter)
    return L.Request(int(mode), int(policy), int(width), int(height), sr[0], sr[1], dr[0], dr[1],
                     iso[0], iso[1], float(rotation_angle))


# Per-request hint / diagnostic bits the debug_* helpers below switch on for every request made through this module (the library
# itself has no process-wide switches: include/aai.h, AAI_POLICY_PREFER_CELL / AAI_POLICY_DIAG_NO_FIXUP)
_extra_policy = 0


def _ref(request):
    """ctypes reference to the request as the library should see it: with the module's extra policy bits, if any"""
    if not _extra_policy:
        return ctypes.byref(request)
    rq = L.Request.from_buffer_copy(request)
    rq.policy |= _extra_policy
    return ctypes.byref(rq)


def last_error():
    return L.load().aai_last_error().decode()


def _check(rc):
    if rc != L.OK:
        raise AaiError(rc, last_error())


def query(request):
    """aai_query: validate + output layout.  Returns (code, message, Layout-or-None).  Needs no GPU."""
    lib = L.load()
    lay = L.Layout()
    rc = lib.aai_query(_ref(request), ctypes.byref(lay))
    if rc != L.OK:
        return rc, last_error(), None
    return rc, "", lay


def device_count():
    n = ctypes.c_int(0)
    L.load().aai_device_count(ctypes.byref(n))
    return n.value


def set_device(ordinal):
    _check(L.load().aai_set_device(int(ordinal)))


def synchronize():
    _check(L.load().aai_device_synchronize())


def last_kernel():
    return L.load().aai_last_kernel().decode()


def _host_forward(a, channels, channel_axis, geometry, entry, *lead, out_dtype=None):
    """Every host forward entry on the prepared image a = [H, W] or [H, W, C], C-contiguous: entry(request, *lead, src, src stride, dst,
    dst stride, layout), strides in elements.  geometry: (src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy);
    channel_axis: the result is [dH, dW, C]; out_dtype: the result's element type where it is not a's.
    Returns (code, message, dst or None, (dstIsoX, dstIsoY) or None, Layout or None)."""
    H, W = a.shape[:2]
    rq = make_request(W, H, *geometry)
    rc, msg, lay = query(rq)
    if rc != L.OK:
        return rc, msg, None, None, None
    dst = np.empty((lay.dst_height, lay.dst_width) + ((channels,) if channel_axis else ()), dtype=out_dtype or a.dtype)
    out_lay = L.Layout()
    rc = entry(_ref(rq), *lead, a.ctypes.data, max(W * channels, 1), dst.ctypes.data, max(lay.dst_width * channels, 1), ctypes.byref(out_lay))
    if rc != L.OK:
        return rc, last_error(), None, None, None
    return rc, "", dst, (out_lay.dst_iso_x, out_lay.dst_iso_y), out_lay


def resample_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle,
                  mode=L.MODE_AREA, policy=L.POLICY_REFERENCE):
    """Host-buffer path (aai_resample_f32 / aai_resample_f64 by dtype).

    Returns (code, message, dst ndarray or None, (dstIsoX, dstIsoY) or None, Layout or None)."""
    lib = L.load()
    a = np.asarray(src)
    geometry = (src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    if a.ndim == 2 and a.dtype in (np.uint8, np.uint16):
        # typed entry (aai_resample_host): 8/16-bit source, fp32 output; the element type goes behind the source pointer
        dt = L.DTYPE_U8 if a.dtype == np.uint8 else L.DTYPE_U16
        return _host_forward(np.ascontiguousarray(a), 1, False, geometry, lambda rq, s, *rest: lib.aai_resample_host(rq, s, dt, *rest), out_dtype=np.float32)
    if a.ndim != 2:
        if a.size != 0:
            raise ValueError("src must be a 2-D image [H, W] (interleaved [H, W, C] images: resample_interleaved_host)")
        a = a.reshape(0, 0)        # the reference's two "no data" errors (Source.cpp:123-132)
    if a.dtype != np.float32:
        a = a.astype(np.float64, copy=False)
    return _host_forward(np.ascontiguousarray(a), 1, False, geometry, lib.aai_resample_f32 if a.dtype == np.float32 else lib.aai_resample_f64)


def precision_check(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE,
                    floor=None):
    """Does THIS image need AAI_POLICY_DOUBLE_PRECISION?  The default kernels take general rotations in fp32 (include/aai.h): a dst
    value is then off by ~5e-8 x the spread of the source values under its footprint, which only shows where a dst value is hundreds
    of times smaller than its neighbours.  That is a property of the data, not of the geometry, so no plan-time scan can flag it:
    this runs the request under both policies and returns (worst relative deviation, dst of the default policy, dst of the
    double-precision policy).  `floor`: absolute floor of the denominator (default 1e-6 x the largest |value|).  A deviation
    above ~1e-5 says: use `policy | POLICY_DOUBLE_PRECISION` for images like this one (about 3 x the time)."""
    rc, msg, fast, _, _ = resample_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=mode, policy=policy)
    if rc != L.OK:
        raise AaiError(rc, msg)
    rc, msg, exact, _, _ = resample_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=mode,
                                        policy=policy | L.POLICY_DOUBLE_PRECISION)
    if rc != L.OK:
        raise AaiError(rc, msg)
    if exact.size == 0:
        return 0.0, fast, exact
    a, b = fast.astype(np.float64), exact.astype(np.float64)
    fl = floor if floor is not None else 1e-6 * max(float(np.abs(b).max()), 1e-300)
    return float((np.abs(a - b) / np.maximum(np.abs(b), fl)).max()), fast, exact


_NP_DTYPES = {np.dtype(np.float32): L.DTYPE_F32, np.dtype(np.uint8): L.DTYPE_U8, np.dtype(np.uint16): L.DTYPE_U16}


class _PinnedBlock:
    """Owner of one hipHostMalloc allocation: freed when the last numpy view of it is gone."""

    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        _check(L.load().aai_host_alloc(ctypes.byref(self.ptr), nbytes))

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr is not None and ptr.value:
            try:
                L.load().aai_host_free(ptr)
            except Exception:           # interpreter shutdown: the runtime may already be gone
                pass


class PinnedArray:
    """A numpy array in page-locked host memory (aai_host_alloc = hipHostMalloc), so that the pipelined host-batch
    entry copies asynchronously.  Use `.array`.  The allocation is owned by the array's base object: close() (or
    leaving the `with` block) only drops this object's reference, and the memory is released when the last numpy view
    of it -- `.array`, slices of it, an `out=` result of resample_batch_host -- has been garbage-collected, so a view
    held elsewhere never dangles."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        block = _PinnedBlock(max(n, 1))
        buf = (ctypes.c_char * max(n, 1)).from_address(block.ptr.value)
        buf._aai_owner = block            # ndarray.base -> buf -> block keeps the allocation alive
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        self.array = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def resample_batch_host(srcs, src_resolution, dst_resolution, src_isocenter, rotation_angle,
                        mode=L.MODE_AREA, policy=L.POLICY_REFERENCE, out=None):
    """Pipelined host-batch path (aai_resample_batch_host): srcs is [B, H, W] float32 / uint8 / uint16 (C-contiguous),
    the result [B, dH, dW] float32 (written into `out` when given, e.g. a PinnedArray's array).
    Returns (code, message, dst or None, Layout or None)."""
    lib = L.load()
    a = np.ascontiguousarray(srcs)
    if a.ndim != 3 or a.dtype not in _NP_DTYPES:
        raise ValueError("srcs must be a [B, H, W] array of float32, uint8 or uint16")
    B, H, W = a.shape
    rq = make_request(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    rc, msg, lay = query(rq)
    if rc != L.OK:
        return rc, msg, None, None
    shape = (B, lay.dst_height, lay.dst_width)
    dst = np.empty(shape, dtype=np.float32) if out is None else out
    if dst.shape != shape or dst.dtype != np.float32 or not dst.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 array of shape %r" % (shape,))
    out_lay = L.Layout()
    rc = lib.aai_resample_batch_host(_ref(rq), B, a.ctypes.data, _NP_DTYPES[a.dtype], W, W * H,
                                     dst.ctypes.data, max(lay.dst_width, 1), lay.dst_width * lay.dst_height, ctypes.byref(out_lay))
    if rc != L.OK:
        return rc, last_error(), None, None
    return rc, "", dst, out_lay


def resample_interleaved_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle,
                              mode=L.MODE_AREA, policy=L.POLICY_REFERENCE):
    """Interleaved channels from host memory (aai_resample_interleaved_host): src is [H, W, C] float32 / uint8 / uint16
    with C in 1..4, the result [dH, dW, C] float32.  Returns (code, message, dst or None, Layout or None)."""
    lib = L.load()
    a = np.ascontiguousarray(src)
    if a.ndim != 3 or a.dtype not in _NP_DTYPES:
        raise ValueError("src must be an [H, W, C] array of float32, uint8 or uint16")
    C = a.shape[2]
    # (the element type goes behind the source pointer)
    rc, msg, dst, _, out_lay = _host_forward(a, C, True, (src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy),
                                             lambda rq, s, *rest: lib.aai_resample_interleaved_host(rq, C, s, _NP_DTYPES[a.dtype], *rest), out_dtype=np.float32)
    return rc, msg, dst, out_lay


def resample_interleaved_device(request, channels, src_ptr, src_stride, dst_ptr, dst_stride, stream=0, batch=1,
                                src_image_stride=0, dst_image_stride=0, src_dtype=L.DTYPE_F32):
    """Device-resident interleaved images (aai_resample_interleaved_device); strides in elements."""
    lib = L.load()
    _check(lib.aai_resample_interleaved_device(_ref(request), int(batch), int(channels), src_ptr, int(src_dtype), src_stride,
                                               src_image_stride, dst_ptr, dst_stride, dst_image_stride, stream))


def resample_device(request, src_ptr, src_stride, dst_ptr, dst_stride, stream=0, batch=None,
                    src_image_stride=0, dst_image_stride=0, src_dtype=L.DTYPE_F32):
    """Device-resident path: raw device pointers (ints) and a hipStream_t handle (int, 0 = default).
    src_dtype: DTYPE_F32 (default) / DTYPE_U8 / DTYPE_U16 -- strides are in source elements."""
    lib = L.load()
    if src_dtype != L.DTYPE_F32:
        _check(lib.aai_resample_batch_device(_ref(request), 1 if batch is None else int(batch), src_ptr, int(src_dtype),
                                             src_stride, src_image_stride, dst_ptr, dst_stride, dst_image_stride, stream))
    elif batch is None:
        _check(lib.aai_resample_device_f32(_ref(request), src_ptr, src_stride, dst_ptr, dst_stride, stream))
    else:
        _check(lib.aai_resample_batch_device_f32(_ref(request), int(batch), src_ptr, src_stride, src_image_stride,
                                                 dst_ptr, dst_stride, dst_image_stride, stream))


# (interleaved entry?, planned kind) -> (device entry, host entry).  The interleaved entries have no ("planned") row: the interleaved
# transposed separable kernel is asked for with "separable" (aai_adjoint_planned_interleaved_*), which is planned at every geometry.
_ADJOINT_ENTRY = {
    (False, "general"): ("aai_adjoint_batch_device_f32", "aai_adjoint_f32"),
    (False, "planned"): ("aai_adjoint_planned_batch_device_f32", "aai_adjoint_planned_f32"),
    (False, "any"): ("aai_adjoint_rotated_batch_device_f32", "aai_adjoint_rotated_f32"),
    (True, "general"): ("aai_adjoint_interleaved_device_f32", "aai_adjoint_interleaved_f32"),
    (True, "any"): ("aai_adjoint_rotated_interleaved_device_f32", "aai_adjoint_rotated_interleaved_f32"),
    (True, "separable"): ("aai_adjoint_planned_interleaved_device_f32", "aai_adjoint_planned_interleaved_f32"),
    # the samplers' adjoint (include/aai_adjoint_sample.h): reached by the adjoint_sample_* wrappers only, never through planned=
    (False, "sample"): ("aai_adjoint_sample_batch_device_f32", "aai_adjoint_sample_f32"),
    (True, "sample"): ("aai_adjoint_sample_interleaved_device_f32", "aai_adjoint_sample_interleaved_f32"),
}


def _planned_kind(planned, interleaved=False):
    """planned=False | True | "any" of the adjoint wrappers -> which family of entries serves the call.  The interleaved wrappers take
    False, "any" or "separable" only; True is refused there, and "separable" by the single-channel wrappers."""
    if interleaved:
        if planned is False:
            return "general"
        if isinstance(planned, str) and planned in ("any", "separable"):
            return planned
        raise ValueError('planned must be False, "any" or "separable" for the interleaved adjoint, got %r' % (planned,))
    if isinstance(planned, str):
        if planned != "any":
            raise ValueError('planned must be False, True or "any", got %r' % (planned,))
        return "any"
    return "planned" if planned else "general"


def _planned_interleaved_kind(planned):
    return _planned_kind(planned, interleaved=True)


def _adjoint_device(interleaved, planned, request, batch, channels, gdst_ptr, dst_stride, dst_image_stride, gsrc_ptr, src_stride, src_image_stride, stream,
                    kind=None):
    """the device entry of _ADJOINT_ENTRY (kind: the family, where the caller names it instead of `planned`); the interleaved entries take
    the channel count after the batch"""
    fn = getattr(L.load(), _ADJOINT_ENTRY[interleaved, kind or _planned_kind(planned, interleaved)][0])
    _check(fn(_ref(request), 1 if batch is None else int(batch), *((int(channels),) if interleaved else ()), gdst_ptr, dst_stride,
              dst_image_stride, gsrc_ptr, src_stride, src_image_stride, stream))


def _adjoint_host(dtype, entry, interleaved, gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy, name="gdst"):
    """Every host adjoint entry on gdst = [dH, dW], or (interleaved) [dH, dW] / [dH, dW, C], of `dtype`: entry(request, C, gdst, gdst
    stride, gsrc, gsrc stride, None) names the C entry and puts C where it takes it -- called last, so that what it raises comes
    behind a failed query and a gdst of the wrong shape (`name` in that text).  Returns (code, message, gsrc or None)."""
    H, W = int(src_shape[0]), int(src_shape[1])
    rq = make_request(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    rc, msg, lay = query(rq)
    if rc != L.OK:
        return rc, msg, None
    g = np.ascontiguousarray(gdst, dtype=dtype)
    tail = g.shape[2:] if interleaved else ()                      # () or (C,)
    C = tail[0] if tail else 1
    if (g.shape[:2] if interleaved else g.shape) != (lay.dst_height, lay.dst_width):
        raise ValueError("%s must have the output's shape %r" % (name, (lay.dst_height, lay.dst_width) + tail))
    gsrc = np.empty((H, W) + tail, dtype=dtype)
    rc = entry(_ref(rq), C, g.ctypes.data, max(lay.dst_width * C, 1), gsrc.ctypes.data, max(W * C, 1), None)
    if rc != L.OK:
        return rc, last_error(), None
    return rc, "", gsrc


def _adjoint_host_f32(interleaved, planned, gdst, *request, kind=None):
    """the fp32 host entry of _ADJOINT_ENTRY; the interleaved entries take the channel count behind the request"""
    lib = L.load()

    def entry(rq, C, *images):
        fn = getattr(lib, _ADJOINT_ENTRY[interleaved, kind or _planned_kind(planned, interleaved)][1])
        return fn(rq, *((C,) if interleaved else ()), *images)
    return _adjoint_host(np.float32, entry, interleaved, gdst, *request)


def adjoint_device(request, gdst_ptr, dst_stride, gsrc_ptr, src_stride, stream=0, batch=None,
                   dst_image_stride=0, src_image_stride=0, planned=False):
    """aai_adjoint_batch_device_f32: gsrc = W(request)^T gdst on device-resident fp32 images -- the transpose of what
    resample_device computes (area and fast modes).  Raw device pointers (ints), strides in elements, a hipStream_t handle;
    every element of the src_width x src_height gradient image is written.
    planned=True: aai_adjoint_planned_batch_device_f32 -- at rotations by multiples of 90 degrees the transposed separable kernel
    on the forward's cached plan (fp32; the first call of a geometry builds the plan's adjoint tables and synchronises, see
    adjoint_prepare), the same general kernels for every other request.
    planned="any": aai_adjoint_rotated_batch_device_f32 -- one entry for every rotation: what planned=True does at multiples of 90
    degrees, and at every other rotation the general adjoint's bits from the plan's cached sums and the plain closed forms (the
    first call of a geometry builds them and synchronises, see adjoint_rotated_prepare)."""
    _adjoint_device(False, planned, request, batch, 1, gdst_ptr, dst_stride, dst_image_stride, gsrc_ptr, src_stride, src_image_stride, stream)


def adjoint_prepare(request):
    """aai_adjoint_prepare: aai_prepare plus the adjoint tables of the plan, so that adjoint_device(..., planned=True) only
    enqueues.  A validated no-op for requests the planned adjoint hands to the general kernels."""
    _check(L.load().aai_adjoint_prepare(_ref(request)))


def adjoint_rotated_prepare(request):
    """aai_adjoint_rotated_prepare: aai_prepare plus the plan's adjoint tables at EVERY rotation -- the sums and knife lists of a general
    rotation (8 bytes per dst pixel on the device), the tables of adjoint_prepare at multiples of 90 degrees -- so that
    adjoint_device(..., planned="any") only enqueues."""
    _check(L.load().aai_adjoint_rotated_prepare(_ref(request)))


def adjoint_host(gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle,
                 mode=L.MODE_AREA, policy=L.POLICY_REFERENCE, planned=False):
    """Host-buffer adjoint (aai_adjoint_f32; planned=True: aai_adjoint_planned_f32; planned="any": aai_adjoint_rotated_f32): gdst is the [dH, dW] gradient with respect to
    the output of resample_host(src of shape src_shape = (H, W), ...); returns (code, message, gsrc [H, W] float32 or None)."""
    return _adjoint_host_f32(False, planned, gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)


def adjoint_interleaved_device(request, channels, gdst_ptr, dst_stride, gsrc_ptr, src_stride, stream=0, batch=None,
                               dst_image_stride=0, src_image_stride=0, planned=False):
    """aai_adjoint_interleaved_device_f32: gsrc = W(request)^T gdst per channel on device-resident fp32 images with `channels` (1..4)
    interleaved channels -- the transpose of what resample_interleaved_device computes (area and fast modes).  Element (x, y, c) of
    image b at b * image_stride + y * stride + x * channels + c; raw device pointers (ints), strides in elements, a hipStream_t
    handle.  Channel c gets the bits adjoint_device gives plane c alone; a pair's weight is computed once for all channels.
    planned="any": aai_adjoint_rotated_interleaved_device_f32 -- the same bits; at a general rotation from the single-channel plan's cached
    sums and the plain closed forms (the first call of a geometry builds them and synchronises, see adjoint_rotated_prepare, which
    serves every channel count), at multiples of 90 degrees the general interleaved kernels.
    planned="separable": aai_adjoint_planned_interleaved_device_f32 -- "any" at every general rotation, and at multiples of 90 degrees
    the interleaved transposed separable kernel (aai_axis_adjoint_multi_kernel<C>, fp32) on the single-channel plan's adjoint tables:
    channel c gets the bits adjoint_device(..., planned=True) gives plane c (adjoint_rotated_prepare builds the tables).
    planned=True raises ValueError: the interleaved wrappers name the path they ask for."""
    _adjoint_device(True, planned, request, batch, channels, gdst_ptr, dst_stride, dst_image_stride, gsrc_ptr, src_stride, src_image_stride, stream)


def adjoint_interleaved_host(gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle,
                             mode=L.MODE_AREA, policy=L.POLICY_REFERENCE, planned=False):
    """Host-buffer interleaved adjoint (aai_adjoint_interleaved_f32; planned="any": aai_adjoint_rotated_interleaved_f32;
    planned="separable": aai_adjoint_planned_interleaved_f32): gdst is the [dH, dW, C] gradient with respect to the output of
    resample_interleaved_host(src of shape (H, W, C), ...), src_shape = (H, W) or (H, W, C); returns (code, message, gsrc [H, W, C]
    float32 or None)."""
    _planned_kind(planned, interleaved=True)                 # (a bad `planned` is reported before a bad gdst)
    g = np.ascontiguousarray(gdst, dtype=np.float32)
    if g.ndim != 3:
        raise ValueError("gdst must be a [dH, dW, C] array")
    if len(src_shape) == 3 and int(src_shape[2]) != g.shape[2]:
        raise ValueError("gdst has %d channels, src_shape %d" % (g.shape[2], int(src_shape[2])))
    return _adjoint_host_f32(True, planned, g, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)


def adjoint_sample_device(request, gdst_ptr, dst_stride, gsrc_ptr, src_stride, stream=0, batch=None, dst_image_stride=0, src_image_stride=0):
    """aai_adjoint_sample_batch_device_f32: gsrc = W(request)^T gdst on device-resident fp32 images for the BILINEAR and BICUBIC modes --
    the transpose of what resample_device computes there (clamp-to-edge taps that add up, zero rows outside the extent, Keys a = -0.5).
    Raw device pointers (ints), strides in elements, a hipStream_t handle; every element of the src_width x src_height gradient image
    is written.  One deterministic gather per source pixel with double-precision weights; no plan, no scratch: the call only enqueues
    and can be captured.  Area and fast requests raise AaiError (their adjoint is adjoint_device)."""
    _adjoint_device(False, False, request, batch, 1, gdst_ptr, dst_stride, dst_image_stride, gsrc_ptr, src_stride, src_image_stride, stream, kind="sample")


def adjoint_sample_host(gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_BILINEAR, policy=L.POLICY_REFERENCE):
    """Host-buffer adjoint of the samplers (aai_adjoint_sample_f32): gdst is the [dH, dW] gradient with respect to the output of
    resample_host(src of shape src_shape = (H, W), ..., mode=MODE_BILINEAR or MODE_BICUBIC); returns (code, message, gsrc [H, W] float32
    or None).  The device entry's bits."""
    return _adjoint_host_f32(False, False, gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy, kind="sample")


def adjoint_sample_interleaved_device(request, channels, gdst_ptr, dst_stride, gsrc_ptr, src_stride, stream=0, batch=None, dst_image_stride=0,
                                      src_image_stride=0):
    """aai_adjoint_sample_interleaved_device_f32: adjoint_sample_device for images with `channels` (1..4) interleaved channels, element
    (x, y, c) of image b at b * image_stride + y * stride + x * channels + c.  Channel c gets the bits adjoint_sample_device gives plane c
    alone; a candidate's weight is computed once for all channels."""
    _adjoint_device(True, False, request, batch, channels, gdst_ptr, dst_stride, dst_image_stride, gsrc_ptr, src_stride, src_image_stride, stream,
                    kind="sample")


def adjoint_sample_interleaved_host(gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_BILINEAR,
                                    policy=L.POLICY_REFERENCE):
    """Host-buffer interleaved adjoint of the samplers (aai_adjoint_sample_interleaved_f32): gdst is the [dH, dW, C] gradient with respect to
    the output of resample_interleaved_host(src of shape (H, W, C), ...), src_shape = (H, W) or (H, W, C); returns (code, message, gsrc
    [H, W, C] float32 or None)."""
    g = np.ascontiguousarray(gdst, dtype=np.float32)
    if g.ndim != 3:
        raise ValueError("gdst must be a [dH, dW, C] array")
    if len(src_shape) == 3 and int(src_shape[2]) != g.shape[2]:
        raise ValueError("gdst has %d channels, src_shape %d" % (g.shape[2], int(src_shape[2])))
    return _adjoint_host_f32(True, False, g, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy, kind="sample")


def resample_device_f64(request, src_ptr, src_stride, dst_ptr, dst_stride, stream=0, batch=None, src_image_stride=0, dst_image_stride=0):
    """aai_resample_batch_device_f64 (include/aai_f64.h): the area / fast forward on device-resident DOUBLE images, never rounded to fp32 --
    the reference's own precision.  Raw device pointers (ints), strides in elements (doubles), a hipStream_t handle; every element of
    the output is written.  No plan, nothing to prepare: the call only enqueues, the first call of a geometry included, and can be
    captured.  Single-channel; bilinear / bicubic requests raise AaiError."""
    _check(L.load().aai_resample_batch_device_f64(_ref(request), 1 if batch is None else int(batch), src_ptr, src_stride, src_image_stride,
                                                  dst_ptr, dst_stride, dst_image_stride, stream))


def adjoint_device_f64(request, gdst_ptr, dst_stride, gsrc_ptr, src_stride, stream=0, batch=None, dst_image_stride=0, src_image_stride=0):
    """aai_adjoint_batch_device_f64 (include/aai_f64.h): gsrc = W(request)^T gdst on device-resident DOUBLE images -- the transpose of
    what resample_device_f64 computes, pair by pair with the same weight bits; adjoint_device's two passes without its final fp32
    rounding.  Raw device pointers (ints), strides in elements (doubles), a hipStream_t handle; every element of the src_width x
    src_height gradient image is written.  No plan: the call only enqueues and can be captured."""
    _check(L.load().aai_adjoint_batch_device_f64(_ref(request), 1 if batch is None else int(batch), gdst_ptr, dst_stride, dst_image_stride,
                                                 gsrc_ptr, src_stride, src_image_stride, stream))


def resample_exact_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE):
    """Host-buffer reference-precision forward (aai_resample_exact_f64): src is a float64 [H, W] image (anything else is converted to
    float64), the result float64 and never rounded to fp32 on the way -- resample_host on a float64 image converts to fp32 on the
    device and widens the fp32 result.  Area and fast modes.  The bits of resample_device_f64.

    Returns (code, message, dst float64 ndarray or None, (dstIsoX, dstIsoY) or None, Layout or None)."""
    lib = L.load()
    a = np.asarray(src)
    if a.ndim != 2:
        if a.size != 0:
            raise ValueError("src must be a 2-D image [H, W]")
        a = a.reshape(0, 0)        # the reference's two "no data" errors (Source.cpp:123-132)
    a = np.ascontiguousarray(a, dtype=np.float64)
    return _host_forward(a, 1, False, (src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy), lib.aai_resample_exact_f64)


def adjoint_exact_host(gdst, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE):
    """Host-buffer reference-precision adjoint (aai_adjoint_f64): gdst is the float64 [dH, dW] gradient with respect to the output of
    resample_exact_host(src of shape src_shape = (H, W), ...); returns (code, message, gsrc [H, W] float64 or None).  The bits of
    adjoint_device_f64."""
    lib = L.load()
    return _adjoint_host(np.float64, lambda rq, C, *images: lib.aai_adjoint_f64(rq, *images), False, gdst, src_shape, src_resolution, dst_resolution,
                         src_isocenter, rotation_angle, mode, policy)


def resample_half_device(request, src_ptr, src_stride, dst_ptr, dst_stride, half_dtype, stream=0, batch=None, src_image_stride=0, dst_image_stride=0):
    """aai_resample_half_batch_device (include/aai_half.h): the forward on device-resident fp16 (half_dtype = HALF_F16) or bf16 (HALF_BF16)
    images, which writes the SAME element type: every source element widened exactly, the forward's fp32 weights and fp32 sums, one
    rounding to nearest-even.  Raw device pointers (ints), strides in 2-byte elements, a hipStream_t handle.  Single-channel, all four
    modes.  The plan is resample_device's (prepare(request, 1) prepares this call too); rotations by 0 / 180 degrees in the area / fast
    modes run one streaming kernel on the half images (last_kernel(): "aai_axis_half_kernel<f16>" / "<bf16>"), everything else widens
    into fp32 scratch, runs resample_device's launches and narrows ("<fp32 kernel>+widened")."""
    _check(L.load().aai_resample_half_batch_device(_ref(request), 1 if batch is None else int(batch), int(half_dtype), src_ptr, src_stride, src_image_stride,
                                                   dst_ptr, dst_stride, dst_image_stride, stream))


def resample_half_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE, half_dtype=None):
    """Host-buffer half-precision forward (aai_resample_half_host): src is a [H, W] image of np.float16 (half_dtype HALF_F16, the default
    for that dtype) or of np.uint16 holding raw bfloat16 bits (HALF_BF16, the default for that dtype); the result has src's dtype.  The
    bits of resample_half_device.

    Returns (code, message, dst ndarray or None, (dstIsoX, dstIsoY) or None, Layout or None)."""
    lib = L.load()
    a = np.asarray(src)
    if a.dtype not in (np.float16, np.uint16):
        raise TypeError("resample_half_host takes np.float16 (fp16) or np.uint16 (raw bf16 bits) images, got %s" % a.dtype)
    if half_dtype is None:
        half_dtype = L.HALF_F16 if a.dtype == np.float16 else L.HALF_BF16
    if a.ndim != 2:
        if a.size != 0:
            raise ValueError("src must be a 2-D image [H, W]")
        a = a.reshape(0, 0)        # the reference's two "no data" errors (Source.cpp:123-132)
    a = np.ascontiguousarray(a)
    return _host_forward(a, 1, False, (src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy), lib.aai_resample_half_host, int(half_dtype))


def resample_half_interleaved_device(request, channels, src_ptr, src_stride, dst_ptr, dst_stride, half_dtype, stream=0, batch=None, src_image_stride=0,
                                     dst_image_stride=0):
    """aai_resample_half_interleaved_device (include/aai_half_interleaved.h): resample_half_device for images of `channels` = 1..4
    interleaved channels -- element (x, y, c) at y * stride + x * channels + c, resample_interleaved_device's layout, which is a
    channels-last tensor's -- read and written in place in the element type.  Raw device pointers (ints), strides in 2-byte elements, a
    hipStream_t handle.  The plan is resample_interleaved_device's (prepare(request, channels) prepares this call too); rotations by
    0 / 180 degrees in the area / fast modes run one streaming kernel (last_kernel(): "aai_axis_half_kernel<f16>" / "<bf16>"),
    everything else widens into fp32 scratch, runs resample_interleaved_device's launches and narrows ("<fp32 kernel>+widened")."""
    _check(L.load().aai_resample_half_interleaved_device(_ref(request), 1 if batch is None else int(batch), int(channels), int(half_dtype), src_ptr, src_stride,
                                                         src_image_stride, dst_ptr, dst_stride, dst_image_stride, stream))


def resample_half_interleaved_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE,
                                   half_dtype=None):
    """Host-buffer half-precision interleaved forward (aai_resample_half_interleaved_host): src is a [H, W, C] (C = 1..4, interleaved) or
    [H, W] image of np.float16 (half_dtype HALF_F16, the default for that dtype) or of np.uint16 holding raw bfloat16 bits (HALF_BF16,
    the default for that dtype); the result has src's dtype and [dH, dW, C] or [dH, dW] shape.  The bits of
    resample_half_interleaved_device.

    Returns (code, message, dst ndarray or None, (dstIsoX, dstIsoY) or None, Layout or None)."""
    lib = L.load()
    a = np.asarray(src)
    if a.dtype not in (np.float16, np.uint16):
        raise TypeError("resample_half_interleaved_host takes np.float16 (fp16) or np.uint16 (raw bf16 bits) images, got %s" % a.dtype)
    if half_dtype is None:
        half_dtype = L.HALF_F16 if a.dtype == np.float16 else L.HALF_BF16
    if a.ndim not in (2, 3):
        if a.size != 0:
            raise ValueError("src must be an image [H, W] or [H, W, C]")
        a = a.reshape(0, 0)        # the reference's two "no data" errors (Source.cpp:123-132)
    a = np.ascontiguousarray(a)
    C = a.shape[2] if a.ndim == 3 else 1
    return _host_forward(a, C, a.ndim == 3, (src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy),
                         lib.aai_resample_half_interleaved_host, C, int(half_dtype))


def adjoint_half_device(request, channels, gdst_ptr, dst_stride, gsrc_ptr, src_stride, half_dtype, stream=0, batch=None, dst_image_stride=0,
                        src_image_stride=0):
    """aai_adjoint_half_device (include/aai_adjoint_half.h): gsrc = W(request)^T gdst on device-resident fp16 (half_dtype = HALF_F16) or
    bf16 (HALF_BF16) gradient images of `channels` = 1..4 interleaved channels, the same element type out -- the transpose of what
    resample_half_interleaved_device computes (area and fast modes).  Raw device pointers (ints), strides in 2-byte elements, a
    hipStream_t handle; every element of gsrc is written.  The bits of narrow(adjoint_interleaved_device(widen(gdst)),
    planned="separable"): at rotations by multiples of 90 degrees on a plan without correction lists ONE launch on the half images
    (last_kernel(): "aai_axis_adjoint_half_kernel<f16|bf16,C>"), everything else widens into fp32 scratch, runs that entry's launches
    and narrows ("<fp32 route>+widened").  adjoint_rotated_prepare(request) prepares these calls."""
    _check(L.load().aai_adjoint_half_device(_ref(request), 1 if batch is None else int(batch), int(channels), int(half_dtype), gdst_ptr, dst_stride,
                                            dst_image_stride, gsrc_ptr, src_stride, src_image_stride, stream))


def adjoint_half_host(gdst_bits, src_shape, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE,
                      half_dtype=None):
    """Host-buffer half-precision adjoint (aai_adjoint_half_host): gdst_bits is the [dH, dW] or [dH, dW, C] (C = 1..4, interleaved)
    gradient as np.uint16 holding the raw bits of half_dtype (HALF_F16 or HALF_BF16; required), src_shape = (H, W); the bits of
    adjoint_half_device.  Returns (code, message, gsrc bits [H, W] or [H, W, C] np.uint16, or None)."""
    lib = L.load()
    if half_dtype is None:
        raise ValueError("adjoint_half_host needs half_dtype (HALF_F16 or HALF_BF16): uint16 bits do not name their type")
    g = np.asarray(gdst_bits)
    if g.dtype != np.uint16:
        raise TypeError("adjoint_half_host takes np.uint16 images of raw fp16 / bf16 bits, got %s" % g.dtype)
    if g.ndim not in (2, 3):
        raise ValueError("gdst_bits must be a [dH, dW] or [dH, dW, C] array")
    return _adjoint_host(np.uint16, lambda rq, C, *images: lib.aai_adjoint_half_host(rq, C, int(half_dtype), *images), True, g, src_shape, src_resolution,
                         dst_resolution, src_isocenter, rotation_angle, mode, policy, name="gdst_bits")


def resample_int_device(request, channels, src_ptr, src_stride, dst_ptr, dst_stride, dtype, stream=0, batch=None, src_image_stride=0, dst_image_stride=0):
    """aai_resample_int_batch_device (include/aai_int.h): the forward on device-resident 8-bit (dtype = DTYPE_U8) or 16-bit (DTYPE_U16)
    unsigned images of `channels` = 1..4 interleaved channels, which writes the SAME element type: every source element as its integer
    value, the forward's fp32 weights and fp32 sums, one conversion -- round to nearest, ties to even, saturate.  Raw device pointers
    (ints), strides in elements, a hipStream_t handle.  All four modes.  The plan is resample_interleaved_device's (prepare(request,
    channels) prepares this call too); rotations by 0 / 180 degrees in the area / fast modes run one streaming kernel on the integer
    images (last_kernel(): "aai_axis_int_kernel<u8>" / "<u16>"), everything else runs resample_interleaved_device's launches into fp32
    scratch and converts ("<fp32 kernel>+quantized")."""
    _check(L.load().aai_resample_int_batch_device(_ref(request), 1 if batch is None else int(batch), int(channels), int(dtype), src_ptr, src_stride,
                                                  src_image_stride, dst_ptr, dst_stride, dst_image_stride, stream))


def resample_int_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE):
    """Host-buffer integer forward (aai_resample_int_host): src is a [H, W] or [H, W, C] (C = 1..4, interleaved) image of np.uint8 or
    np.uint16; the result has src's dtype and [dH, dW] or [dH, dW, C] shape.  The bits of resample_int_device.

    Returns (code, message, dst ndarray or None, (dstIsoX, dstIsoY) or None, Layout or None)."""
    lib = L.load()
    a = np.asarray(src)
    if a.dtype not in (np.uint8, np.uint16):
        raise TypeError("resample_int_host takes np.uint8 or np.uint16 images, got %s" % a.dtype)
    dtype = L.DTYPE_U8 if a.dtype == np.uint8 else L.DTYPE_U16
    if a.ndim not in (2, 3):
        if a.size != 0:
            raise ValueError("src must be an image [H, W] or [H, W, C]")
        a = a.reshape(0, 0)        # the reference's two "no data" errors (Source.cpp:123-132)
    a = np.ascontiguousarray(a)
    C = a.shape[2] if a.ndim == 3 else 1
    return _host_forward(a, C, a.ndim == 3, (src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy), lib.aai_resample_int_host, C, dtype)


def make_convert(channels, out_type=L.DTYPE_F32, planar=False, scale=None, offset=None):
    """aai_convert (include/ext/aai_convert.h) for `channels` channels: out_type DTYPE_F32, HALF_F16 or HALF_BF16; scale / offset a scalar or
    one value per channel (default 1 and 0)"""
    def per_channel(v, default):
        v = default if v is None else v
        vals = [float(v)] * channels if np.ndim(v) == 0 else [float(x) for x in v]
        if len(vals) != channels:
            raise ValueError("scale and offset take a scalar or one value per channel (%d), got %d" % (channels, len(vals)))
        return vals + [0.0] * (4 - len(vals))
    if not 1 <= int(channels) <= 4:
        raise ValueError("channels must be 1..4")
    cv = L.Convert()
    cv.out_type, cv.out_layout = int(out_type), L.LAYOUT_PLANAR if planar else L.LAYOUT_INTERLEAVED
    cv.scale[:] = per_channel(scale, 1.0)
    cv.offset[:] = per_channel(offset, 0.0)
    return cv


_CONVERT_NP = {L.DTYPE_F32: np.float32, L.HALF_F16: np.float16, L.HALF_BF16: np.uint16}      # (bf16: raw 16-bit elements)


def resample_convert_device(request, channels, src_ptr, src_stride, dst_ptr, dst_stride, src_dtype, convert, stream=0, batch=None, src_image_stride=0,
                            dst_image_stride=0, dst_plane_stride=0):
    """aai_resample_convert_device (include/ext/aai_convert.h): device-resident 8-bit (src_dtype = DTYPE_U8) or 16-bit (DTYPE_U16) unsigned
    images of `channels` = 1..4 interleaved channels in, round(fma(resample(src), scale[c], offset[c])) out in convert.out_type, interleaved
    or planar (make_convert).  Raw device pointers (ints), strides in elements of the respective type, a hipStream_t handle.  All four
    modes.  Rotations by 0 / 180 degrees in the area / fast modes run one kernel from the integer image to the converted image
    (last_kernel(): "aai_axis_convert_kernel<u8|u16,f32|f16|bf16>"), everything else runs resample_interleaved_device's launches into fp32
    scratch and converts ("<fp32 kernel>+converted")."""
    _check(L.load().aai_resample_convert_device(_ref(request), 1 if batch is None else int(batch), int(channels), int(src_dtype), src_ptr, src_stride,
                                                src_image_stride, ctypes.byref(convert) if convert is not None else None, dst_ptr, dst_stride, dst_plane_stride,
                                                dst_image_stride, stream))


def resample_convert_host(src, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode=L.MODE_AREA, policy=L.POLICY_REFERENCE, out_type=L.DTYPE_F32,
                          planar=False, scale=None, offset=None):
    """Host-buffer resample-and-convert (aai_resample_convert_host): src is a [H, W] or [H, W, C] (C = 1..4, interleaved) image of np.uint8 or
    np.uint16; the result is [dH, dW, C] (interleaved; [dH, dW] for a 2-D src) or [C, dH, dW] (planar) of np.float32, np.float16 or -- bf16 --
    raw np.uint16 elements.  The bits of resample_convert_device.

    Returns (code, message, dst ndarray or None, (dstIsoX, dstIsoY) or None, Layout or None)."""
    lib = L.load()
    a = np.asarray(src)
    if a.dtype not in (np.uint8, np.uint16):
        raise TypeError("resample_convert_host takes np.uint8 or np.uint16 images, got %s" % a.dtype)
    if out_type not in _CONVERT_NP:
        raise ValueError("out_type must be DTYPE_F32, HALF_F16 or HALF_BF16")
    dtype = L.DTYPE_U8 if a.dtype == np.uint8 else L.DTYPE_U16
    if a.ndim not in (2, 3):
        if a.size != 0:
            raise ValueError("src must be an image [H, W] or [H, W, C]")
        a = a.reshape(0, 0)        # the reference's two "no data" errors (Source.cpp:123-132)
    a = np.ascontiguousarray(a)
    H, W = a.shape[:2]
    C = a.shape[2] if a.ndim == 3 else 1
    cv = make_convert(C, out_type, planar, scale, offset)
    rq = make_request(W, H, src_resolution, dst_resolution, src_isocenter, rotation_angle, mode, policy)
    rc, msg, lay = query(rq)
    if rc != L.OK:
        return rc, msg, None, None, None
    dH, dW = lay.dst_height, lay.dst_width
    dst = np.empty((C, dH, dW) if planar else ((dH, dW, C) if a.ndim == 3 else (dH, dW)), dtype=_CONVERT_NP[out_type])
    out_lay = L.Layout()
    rc = lib.aai_resample_convert_host(_ref(rq), C, dtype, a.ctypes.data, max(W * C, 1), ctypes.byref(cv), dst.ctypes.data, max(dW if planar else dW * C, 1),
                                       max(dW * dH, 1), ctypes.byref(out_lay))
    if rc != L.OK:
        return rc, last_error(), None, None, None
    return rc, "", dst, (out_lay.dst_iso_x, out_lay.dst_iso_y), out_lay


def resample_multi_device(request, shards, src_stride, src_image_stride, dst_stride, dst_image_stride):
    """aai_resample_batch_multi_device_f32: `shards` is a list of (device, count, src_ptr, dst_ptr, stream) -- one batch of
    independent images spread over several GPUs of this process, no collective."""
    n = len(shards)
    devs = (ctypes.c_int32 * n)(*[int(s[0]) for s in shards])
    cnts = (ctypes.c_int32 * n)(*[int(s[1]) for s in shards])
    srcs = (ctypes.c_void_p * n)(*[s[2] for s in shards])
    dsts = (ctypes.c_void_p * n)(*[s[3] for s in shards])
    strs = (ctypes.c_void_p * n)(*[s[4] for s in shards])
    _check(L.load().aai_resample_batch_multi_device_f32(_ref(request), n, devs, cnts, srcs, src_stride, src_image_stride,
                                                       dsts, dst_stride, dst_image_stride, strs))


def band_source_rows(request, dst_row0, dst_row1):
    """aai_band_source_rows: source rows [a, b) that dst rows [dst_row0, dst_row1) read.  Needs no GPU."""
    a, b = ctypes.c_int32(), ctypes.c_int32()
    _check(L.load().aai_band_source_rows(_ref(request), int(dst_row0), int(dst_row1), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def resample_band_device(request, dst_row0, dst_row1, src_rows_ptr, src_stride, dst_rows_ptr, dst_stride, stream=0):
    """aai_resample_band_device_f32: src_rows_ptr addresses source row band_source_rows(...)[0], dst_rows_ptr output row dst_row0."""
    _check(L.load().aai_resample_band_device_f32(_ref(request), int(dst_row0), int(dst_row1), src_rows_ptr, src_stride,
                                                 dst_rows_ptr, dst_stride, stream))


def plan_shape(request, channels=1):
    """aai_plan_info: one line describing the cached whole-image plan of this request on the current device ("" if none):
    kernel family, K1 launch shape and its origin, flagged pixels, fp32 formulation, build time, adjoint tables (tables | none), and last the tables of the planned adjoint at general rotations
    (rot_adjoint=none | sums | general, then knife=<count> once its scan has run)."""
    buf = ctypes.create_string_buffer(512)
    _check(L.load().aai_plan_info(_ref(request), int(channels), buf, 512))
    return buf.value.decode()


def debug_cell_min_waves(waves):
    """tests: 0 = every rotated area request made through this module carries AAI_POLICY_PREFER_CELL (small outputs take the cell
    kernel too); anything else = the default (outputs below ~720 x 720 pixels stay on the quad kernel)"""
    global _extra_policy
    _extra_policy = (_extra_policy | L.POLICY_PREFER_CELL) if int(waves) == 0 else (_extra_policy & ~L.POLICY_PREFER_CELL)


def debug_skip_fixup(skip):
    """tests / timing: True = requests made through this module carry AAI_POLICY_DIAG_NO_FIXUP (the double-precision fix-up pass is
    not launched, the plan's listed pixels keep the caller's bytes)"""
    global _extra_policy
    _extra_policy = (_extra_policy | L.POLICY_DIAG_NO_FIXUP) if skip else (_extra_policy & ~L.POLICY_DIAG_NO_FIXUP)


def shutdown():
    """aai_shutdown: drop every cached plan now (optional; a process may simply exit)."""
    L.load().aai_shutdown()


def prepare(request, channels=1):
    """aai_prepare: build (and cache) the plan of this request on the current device now -- K1 tables, the one-off
    scans of a rotated geometry -- instead of inside the first resampling call, which would then synchronise."""
    _check(L.load().aai_prepare(_ref(request), int(channels)))


def synth_rows_device(dst_ptr, width, height, row0, row1, stride, seed, stream=0):
    """rows [row0, row1) of the synthetic width x height image; dst_ptr addresses row row0"""
    _check(L.load().aai_synth_rows_device_f32(dst_ptr, int(width), int(height), int(row0), int(row1), int(stride), int(seed), stream))


def synth_device(dst_ptr, width, height, stride, seed, stream=0):
    _check(L.load().aai_synth_device_f32(dst_ptr, int(width), int(height), int(stride), int(seed), stream))


class AreaAverageInterpolation:
    """Stateless, like the reference class (no data members, Source.cpp:52-54)."""

    def __init__(self, policy=L.POLICY_REFERENCE, exact=False):
        """exact=True: areaAverageInterpolation and fastAreaAverageInterpolation run in the reference's own precision (resample_exact_host:
        double images end to end, dst is float64 whatever src's dtype); the two sampler methods are unchanged."""
        self.policy = policy
        self.exact = bool(exact)

    def _call(self, mode, src, srcResolution, dstResolution, srcIsocenter, rotationAngle):
        host = resample_exact_host if self.exact and mode in (L.MODE_AREA, L.MODE_FAST) else resample_host
        rc, msg, dst, iso, _ = host(src, srcResolution, dstResolution, srcIsocenter, rotationAngle, mode=mode, policy=self.policy)
        if rc in (L.ERR_RESOLUTION_MISMATCH, L.ERR_RESOLUTION_NONPOSITIVE, L.ERR_NO_ROWS, L.ERR_NO_COLUMNS):
            return (False, msg), None, None          # the reference's {false, message}
        if rc != L.OK:
            raise AaiError(rc, msg)                  # conditions the reference cannot report
        return (True, ""), dst, iso

    def areaAverageInterpolation(self, src, srcResolution, dstResolution, srcIsocenter, rotationAngle):
        """Source.cpp:55"""
        return self._call(L.MODE_AREA, src, srcResolution, dstResolution, srcIsocenter, rotationAngle)

    def fastAreaAverageInterpolation(self, src, srcResolution, dstResolution, srcIsocenter, rotationAngle):
        """Source.cpp:584"""
        return self._call(L.MODE_FAST, src, srcResolution, dstResolution, srcIsocenter, rotationAngle)

    # build-defined comparison paths (README.md:8 of the reference names them; it implements neither)
    def bilinearInterpolation(self, src, srcResolution, dstResolution, srcIsocenter, rotationAngle):
        return self._call(L.MODE_BILINEAR, src, srcResolution, dstResolution, srcIsocenter, rotationAngle)

    def bicubicInterpolation(self, src, srcResolution, dstResolution, srcIsocenter, rotationAngle):
        return self._call(L.MODE_BICUBIC, src, srcResolution, dstResolution, srcIsocenter, rotationAngle)
