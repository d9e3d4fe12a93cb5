// aai_capi.cpp -- the C ABI declared in include/aai.h: the extern "C" entry points and the host-buffer convenience
// paths, on top of the engine (aai_engine.cpp: plan cache, dispatch, error state).
//
// There is deliberately no CPU implementation behind this ABI: without a HIP device every compute entry
// point fails with AAI_ERR_NO_DEVICE.  The CPU oracle under oracle/ is test infrastructure and is never
// linked or loaded here.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <list>
#include <mutex>
#include <string>
#include <vector>

#include "aai_engine.hpp"
#include "../../include/aai_adjoint_planned.h"
#include "../../include/aai_adjoint_interleaved.h"
#include "../../include/aai_adjoint_rotated.h"
#include "../../include/aai_adjoint_rotated_interleaved.h"
#include "../../include/aai_adjoint_planned_interleaved.h"
#include "../../include/aai_adjoint_sample.h"
#include "../../include/aai_f64.h"
#include "../../include/aai_half.h"
#include "../../include/aai_half_interleaved.h"
#include "../../include/aai_adjoint_half.h"
#include "../../include/aai_int.h"
#include "../../include/ext/aai_convert.h"

using namespace aai::engine;

namespace {

// ---- argument checks ---------------------------------------------------------------------------------------
// An entry point reads as the list of its checks: each returns AAI_OK or records its text and returns its code, and the
// first that fails ends the call.  Argument errors come before the device is touched, like the reference reports them
// first; the ORDER of an entry point's checks is what a caller with two faults sees and is pinned, entry point by entry
// point, by tests/test_entry_point_errors.py -- which is why check_request and request_geometry are two calls: most
// entry points report a bad element type, channel count or batch between the two.
#define AAI_TRY(check)                              \
    do {                                            \
        const int rc__ = (check);                   \
        if (rc__ != AAI_OK) return rc__;            \
    } while (0)

int request_geometry(const aai_request &rq, aai::Geometry &g)      // the reference's validation and everything derived from the request
{
    std::string msg;
    const int rc = aai::make_geometry(rq, g, msg);
    return rc == AAI_OK ? AAI_OK : fail(rc, msg);
}

int check_dtype(int32_t dtype)
{
    if (dtype != AAI_DTYPE_F32 && dtype != AAI_DTYPE_U8 && dtype != AAI_DTYPE_U16) return fail(AAI_ERR_BAD_ARGUMENT, "Unknown source element type.");
    return AAI_OK;
}

int check_half_dtype(int32_t dtype)      // include/aai_half.h, aai_half_interleaved.h, aai_adjoint_half.h
{
    if (dtype != AAI_HALF_F16 && dtype != AAI_HALF_BF16) return fail(AAI_ERR_BAD_ARGUMENT, "Unknown half-precision element type.");
    return AAI_OK;
}

int check_int_dtype(int32_t dtype)      // include/aai_int.h
{
    if (dtype != AAI_DTYPE_U8 && dtype != AAI_DTYPE_U16) return fail(AAI_ERR_BAD_ARGUMENT, "Unknown integer element type.");
    return AAI_OK;
}

int check_channels(int32_t channels)
{
    return channels < 1 || channels > 4 ? fail(AAI_ERR_BAD_ARGUMENT, "Channels must be 1..4.") : AAI_OK;
}

int check_batch(int32_t batch)      // any size: enqueue() splits batches beyond the grid.z limit
{
    return batch < 0 ? fail(AAI_ERR_BAD_ARGUMENT, "Negative batch.") : AAI_OK;
}

int check_pointers(const void *a, const void *b)
{
    return !a || !b ? fail(AAI_ERR_BAD_ARGUMENT, "Null image pointer.") : AAI_OK;
}

// interleaved images: the kernels index the elements of a row with 32-bit integers
int check_row_length(const aai::Geometry &g, int channels)
{
    if ((int64_t)g.W * channels > INT32_MAX / 2 || (int64_t)g.dW * channels > INT32_MAX / 2) return fail(AAI_ERR_TOO_LARGE, "Image too large.");
    return AAI_OK;
}

// strides in elements; an interleaved pixel takes `channels` of them
int check_strides(const aai::Geometry &g, int channels, int64_t srcStride, int64_t dstStride)
{
    if (srcStride < (int64_t)g.W * channels) return fail(AAI_ERR_BAD_ARGUMENT, "Source stride smaller than the image width.");
    if (dstStride < (int64_t)g.dW * channels) return fail(AAI_ERR_BAD_ARGUMENT, "Destination stride smaller than the output width.");
    return AAI_OK;
}

// The adjoint of an area / fast request: the argument checks of every adjoint entry, none of which needs a device -- the request's
// part (all aai_adjoint_prepare has to check) ...  `subject` names the caller in the texts: the forward of include/aai_f64.h takes
// the same modes and runs the same checks (check_f64_forward).
int check_adjoint_request(const aai_request *rq, int batch, aai::Geometry &g, const char *subject = "adjoint")
{
    AAI_TRY(check_request(rq));
    AAI_TRY(check_batch(batch));
    AAI_TRY(request_geometry(*rq, g));
    const std::string no = std::string("No ") + subject + " for ";
    if (rq->mode == AAI_MODE_BILINEAR) return fail(AAI_ERR_BAD_ARGUMENT, no + "AAI_MODE_BILINEAR: the area and fast modes only.");
    if (rq->mode == AAI_MODE_BICUBIC) return fail(AAI_ERR_BAD_ARGUMENT, no + "AAI_MODE_BICUBIC: the area and fast modes only.");
    if (rq->policy & AAI_POLICY_DIAG_NO_FIXUP) return fail(AAI_ERR_BAD_ARGUMENT, std::string("AAI_POLICY_DIAG_NO_FIXUP has no meaning for the ") + subject + ".");
    return AAI_OK;
}
// Its sibling for the samplers' adjoint (include/aai_adjoint_sample.h): ONLY the bilinear and bicubic modes.  The policy's rule and bits are
// validated (check_request, as aai_query validates them) and otherwise ignored, as the forward's samplers ignore them.
int check_adjoint_sample_request(const aai_request *rq, int batch, aai::Geometry &g)
{
    AAI_TRY(check_request(rq));
    AAI_TRY(check_batch(batch));
    AAI_TRY(request_geometry(*rq, g));
    if (rq->mode == AAI_MODE_AREA) return fail(AAI_ERR_BAD_ARGUMENT, "The adjoint of AAI_MODE_AREA is aai_adjoint_batch_device_f32: the bilinear and bicubic modes only.");
    if (rq->mode == AAI_MODE_FAST) return fail(AAI_ERR_BAD_ARGUMENT, "The adjoint of AAI_MODE_FAST is aai_adjoint_batch_device_f32: the bilinear and bicubic modes only.");
    return AAI_OK;
}
// ... and the images'.  The interleaved entries (aai_adjoint_interleaved_*, aai_adjoint_rotated_interleaved_*, aai_adjoint_planned_interleaved_*) check the channel count
// right after the request, as the forward's interleaved entries report it, and the row length before the pointers; the single-channel
// entries check neither.  Strides in elements of `channels` per pixel.
// (halfDtype: the element type of the entries of include/aai_adjoint_half.h, checked directly behind the channel count; NULL: the fp32 and
// f64 entries, which have none)
int check_adjoint(AdjointFamily family, const aai_request *rq, int batch, bool interleaved, int channels, const int32_t *halfDtype, const void *gdst,
                  int64_t dstStride, const void *gsrc, int64_t srcStride, aai::Geometry &g)
{
    if (interleaved) {
        AAI_TRY(check_request(rq));
        AAI_TRY(check_channels(channels));
        if (halfDtype) AAI_TRY(check_half_dtype(*halfDtype));
    }
    AAI_TRY(family == ADJOINT_SAMPLE ? check_adjoint_sample_request(rq, batch, g) : check_adjoint_request(rq, batch, g));
    if (interleaved) AAI_TRY(check_row_length(g, channels));
    AAI_TRY(check_pointers(gdst, gsrc));
    return check_strides(g, channels, srcStride, dstStride);
}

// The forward of the reference-precision path (include/aai_f64.h): the checks of a single-channel general adjoint, check for check, in
// its order and with its messages where they apply (the adjoint entries of aai_f64.h run check_adjoint itself).
int check_f64_forward(const aai_request *rq, int batch, const void *src, int64_t srcStride, const void *dst, int64_t dstStride, aai::Geometry &g)
{
    AAI_TRY(check_adjoint_request(rq, batch, g, "f64 forward"));
    AAI_TRY(check_pointers(src, dst));
    return check_strides(g, 1, srcStride, dstStride);
}

// ---- the tail of a device entry ----------------------------------------------------------------------------------------------
// The argument checks done: (an empty batch is done, without a look at the device;) the device check; `late`, a check the entry
// reports from behind the device check; `run`, its enqueue; a clean error text.  Two variations live in the arguments and are pinned
// by the recordings of tests/test_entry_point_errors.py ("The entry layer"):
//   emptyBatch  `batch == 0` from the entries that have the shortcut, `false` from those that do not: the fp32 forward entries, whose
//               empty batch goes on to the device check and into enqueue()
//   late        the strides of the half / integer device entries, which stand where the fp32 forward entries report theirs: in enqueue()
template <typename Late, typename Run>
int device_tail(bool emptyBatch, Late late, Run run)
{
    if (!emptyBatch) {
        AAI_TRY(require_device());
        AAI_TRY(late());
        AAI_TRY(run());
    }
    g_lastError.clear();
    return AAI_OK;
}
template <typename Run>
int device_tail(bool emptyBatch, Run run)
{
    return device_tail(emptyBatch, [] { return (int)AAI_OK; }, run);
}

// every device entry of the adjoint; the single-channel entries pass interleaved = false, channels = 1
int adjoint_device(AdjointFamily family, bool interleaved, const aai_request *req, int32_t batch, int32_t channels, const float *d_gdst,
                   int64_t dst_stride, int64_t dst_image_stride, float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_adjoint(family, req, batch, interleaved, channels, nullptr, d_gdst, dst_stride, d_gsrc, src_stride, g));
    return device_tail(batch == 0, [&] {
        return enqueue_adjoint(family, *req, g, batch, channels, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, (hipStream_t)stream);
    });
}

// aai_adjoint_prepare / aai_adjoint_rotated_prepare
int adjoint_prepare(AdjointFamily family, const aai_request *req)
{
    aai::Geometry g;
    AAI_TRY(check_adjoint_request(req, 1, g));
    return device_tail(false, [&] { return enqueue_adjoint(family, *req, g, 0, 1, nullptr, 0, 0, nullptr, 0, 0, nullptr); });
}

int finish(const aai_request &rq, const aai::Geometry &g, aai_layout *layout)
{
    if (layout) fill_layout(g, resolved_kernel(rq, g), layout);
    g_lastError.clear();
    return AAI_OK;
}

// ---- host-buffer paths -------------------------------------------------------------------------------------
// a hipMalloc allocation that frees itself (move-only)
struct DeviceBuffer {
    void *p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p(o.p) { o.p = nullptr; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(p, o.p); return *this; }
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }      // (no padding: every kernel clamps its vector loads into the image)
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// One image of a host round trip: the caller's strided rows and the dense rows of their twin on the device.  Sizes in elements of
// `esz` bytes.  (src_image / dst_image: the request's source and output with `channels` interleaved elements per pixel.  An adjoint
// reads a dst_image, gdst, and writes a src_image, gsrc.)
struct HostImage {
    void *p;
    int64_t stride, row;
    int rows;
    size_t esz;
    size_t bytes() const { return esz * (size_t)row * (size_t)rows; }
};
HostImage src_image(const aai::Geometry &g, int channels, const void *p, int64_t stride, size_t esz)
{
    return {const_cast<void *>(p), stride, (int64_t)g.W * channels, g.H, esz};
}
HostImage dst_image(const aai::Geometry &g, int channels, const void *p, int64_t stride, size_t esz)
{
    return {const_cast<void *>(p), stride, (int64_t)g.dW * channels, g.dH, esz};
}

// THE host round trip, behind every host entry but the pipelined aai_resample_batch_host, the caller's checks done: two dense device
// images, `in` uploaded, run(dIn, dOut, stream) -> int enqueues once on the null stream, synchronise, `out` downloaded, finish().
// launchWhenEmpty says what an output without elements means ("The entry layer", has the table): true = nothing is
// skipped (the adjoint entries); false = the input still goes up, and the output's allocation, run(), the wait and the download are
// skipped (the fp32 forward entries).  An entry that returns before it touches the allocator says so itself, in front of this call.
template <typename Run>
int round_trip(const aai_request &rq, const aai::Geometry &g, const HostImage &in, const HostImage &out, bool launchWhenEmpty, aai_layout *layout, Run run)
{
    const bool launch = launchWhenEmpty || out.bytes() != 0;
    DeviceBuffer dIn, dOut;
    hipStream_t stream = nullptr;
    AAI_HIP(dIn.alloc(in.bytes()));
    if (launch) AAI_HIP(dOut.alloc(out.bytes()));
    AAI_HIP(hipMemcpy2D(dIn.p, in.esz * in.row, in.p, in.esz * in.stride, in.esz * in.row, in.rows, hipMemcpyHostToDevice));
    if (launch) {
        AAI_TRY(run(dIn.p, dOut.p, stream));
        AAI_HIP(hipStreamSynchronize(stream));
        AAI_HIP(hipMemcpy2D(out.p, out.esz * out.stride, dOut.p, out.esz * out.row, out.esz * out.row, out.rows, hipMemcpyDeviceToHost));
    }
    return finish(rq, g, layout);
}

// aai_resample_f32 / _f64 / _host / _interleaved_host.  srcType: AAI_DTYPE_* of the host source; f64: host source AND destination are
// doubles instead, converted to and from fp32 on the device.  Strides in elements.
int host_round_trip(const aai_request &rq, const aai::Geometry &g, int channels, int srcType, bool f64, const void *src, int64_t srcStride,
                    void *dst, int64_t dstStride, aai_layout *layout)
{
    const HostImage in = src_image(g, channels, src, srcStride, f64 ? sizeof(double) : aai::src_elem_size(srcType));
    const HostImage out = dst_image(g, channels, dst, dstStride, f64 ? sizeof(double) : sizeof(float));
    const size_t nSrc = (size_t)in.row * g.H, nDst = (size_t)out.row * g.dH;
    DeviceBuffer in32, out32;      // the fp32 source and result of a double-precision call (freed behind the round trip's wait)
    return round_trip(rq, g, in, out, /*launchWhenEmpty*/ false, layout, [&](const void *dIn, void *dOut, hipStream_t stream) -> int {
        if (!f64) return enqueue(rq, g, 1, dIn, srcType, in.row, 0, static_cast<float *>(dOut), out.row, 0, stream, -1, -1, channels);
        AAI_HIP(in32.alloc(sizeof(float) * nSrc));
        AAI_HIP(out32.alloc(sizeof(float) * nDst));
        AAI_HIP(aai::launch_f64_to_f32(static_cast<const double *>(dIn), in32.as<float>(), nSrc, stream));
        AAI_TRY(enqueue(rq, g, 1, in32.p, aai::SRC_F32, in.row, 0, out32.as<float>(), out.row, 0, stream, -1, -1, channels));
        AAI_HIP(aai::launch_f32_to_f64(out32.as<const float>(), static_cast<double *>(dOut), nDst, stream));
        return AAI_OK;
    });
}

// aai_resample_half_host / _half_interleaved_host / _int_host: the element type in, the same type out; an output without elements
// returns before the allocator is touched
template <typename Run>
int narrow_round_trip(const aai_request &rq, const aai::Geometry &g, int channels, size_t esz, const void *src, int64_t srcStride, void *dst, int64_t dstStride,
                      aai_layout *layout, Run run)
{
    const HostImage in = src_image(g, channels, src, srcStride, esz), out = dst_image(g, channels, dst, dstStride, esz);
    if (!out.bytes()) return finish(rq, g, layout);
    return round_trip(rq, g, in, out, true, layout, run);
}

// aai_resample_f32 / aai_resample_f64
int resample_host_plain(const aai_request *req, bool f64, const void *src, int64_t srcStride, void *dst, int64_t dstStride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_strides(g, 1, srcStride, dstStride));
    AAI_TRY(require_device());
    return host_round_trip(*req, g, 1, AAI_DTYPE_F32, f64, src, srcStride, dst, dstStride, layout);
}

// validates the request and a dst row band; the source rows the band reads
int band_source_rows(const aai_request *req, int32_t dst_row0, int32_t dst_row1, int32_t *src_row0, int32_t *src_row1, aai::Geometry &g)
{
    AAI_TRY(check_request(req));
    if (!src_row0 || !src_row1) return fail(AAI_ERR_BAD_ARGUMENT, "Null output pointer.");
    AAI_TRY(request_geometry(*req, g));
    if (dst_row0 < 0 || dst_row1 > g.dH || dst_row0 >= dst_row1) return fail(AAI_ERR_BAD_ARGUMENT, "Band rows out of range.");
    const int kernel = pick_kernel(*req, g);
    int a = 0, b = g.H;
    if (kernel == AAI_KERNEL_AXIS) {
        aai::AxisTables t;
        aai::build_axis_tables(g, req->mode, t);
        aai::restrict_axis_tables_to_band(g, t, dst_row0, dst_row1, a, b, axis_band_margin(*req));
    } else {
        if (dst_row0 % 16 != 0) return fail(AAI_ERR_BAD_ARGUMENT, "Band start must be a multiple of 16 rows for rotated requests.");
        aai::rotated_band_source_rows(g, dst_row0, dst_row1, kernel == AAI_KERNEL_SAMPLE, a, b);
    }
    *src_row0 = a; *src_row1 = b;
    g_lastError.clear();
    return AAI_OK;
}

// Device slots of the pipelined host-batch entry, kept between calls (allocating and freeing ~100 MB buffers costs
// about as much as moving one 8-bit image over PCIe).  One pool per process; calls are serialised on its mutex.
constexpr int kSlots = 3;
struct SlotPool {
    int device = -1;
    size_t srcBytes = 0, dstBytes = 0;
    hipStream_t streams[kSlots] = {nullptr, nullptr, nullptr};
    void *dSrc[kSlots] = {nullptr, nullptr, nullptr};
    float *dDst[kSlots] = {nullptr, nullptr, nullptr};
    void release()
    {
        for (int s = 0; s < kSlots; ++s) {
            if (streams[s]) { (void)hipStreamSynchronize(streams[s]); (void)hipStreamDestroy(streams[s]); streams[s] = nullptr; }
            if (dSrc[s]) { (void)hipFree(dSrc[s]); dSrc[s] = nullptr; }
            if (dDst[s]) { (void)hipFree(dDst[s]); dDst[s] = nullptr; }
        }
        srcBytes = dstBytes = 0; device = -1;
    }
    hipError_t reserve(size_t needSrc, size_t needDst)
    {
        int dev = -1;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev == device && needSrc <= srcBytes && needDst <= dstBytes) return hipSuccess;
        release();
        for (int s = 0; s < kSlots && e == hipSuccess; ++s) {
            e = hipStreamCreateWithFlags(&streams[s], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipMalloc(&dSrc[s], needSrc);
            if (e == hipSuccess) e = hipMalloc((void **)&dDst[s], needDst);
        }
        if (e != hipSuccess) { release(); return e; }
        device = dev; srcBytes = needSrc; dstBytes = needDst;
        return hipSuccess;
    }
};
std::mutex g_slotMutex;
SlotPool g_slots;

// page-locked (hipHostMalloc / hipHostRegister) memory copies asynchronously; anything else is staged by the runtime
bool is_page_locked(const void *p)
{
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost;
}

// every fp32 host entry of the adjoint: gdst up, one launch, gsrc down; the single-channel entries pass interleaved = false, channels = 1
int adjoint_host(AdjointFamily family, bool interleaved, const aai_request *req, int channels, const float *gdst, int64_t dst_stride, float *gsrc,
                 int64_t src_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_adjoint(family, req, 1, interleaved, channels, nullptr, gdst, dst_stride, gsrc, src_stride, g));
    AAI_TRY(require_device());
    const HostImage in = dst_image(g, channels, gdst, dst_stride, sizeof(float)), out = src_image(g, channels, gsrc, src_stride, sizeof(float));
    return round_trip(*req, g, in, out, /*launchWhenEmpty*/ true, layout, [&](const void *dGdst, void *dGsrc, hipStream_t stream) {
        return enqueue_adjoint(family, *req, g, 1, channels, static_cast<const float *>(dGdst), in.row, 0, static_cast<float *>(dGsrc), out.row, 0, stream);
    });
}

}  // namespace

extern "C" {

int aai_version(void) { return AAI_VERSION_MAJOR * 1000 + AAI_VERSION_MINOR; }

const char *aai_last_error(void) { return g_lastError.c_str(); }

const char *aai_last_kernel(void) { return g_lastKernel.c_str(); }

const char *aai_error_string(int code)
{
    switch (code) {
    case AAI_OK: return "";
    case AAI_ERR_RESOLUTION_MISMATCH: return "Assumed X & Y resolution are same.";
    case AAI_ERR_RESOLUTION_NONPOSITIVE: return "0 or negative resolution is not acceptable.";
    case AAI_ERR_NO_ROWS: return "There is no data in src array.";
    case AAI_ERR_NO_COLUMNS: return "There is no data in the second dimension of src array.";
    case AAI_ERR_NONFINITE: return "Non-finite argument.";
    case AAI_ERR_BAD_ARGUMENT: return "Bad argument.";
    case AAI_ERR_TOO_LARGE: return "Image too large.";
    case AAI_ERR_NO_DEVICE: return "No HIP device available.";
    case AAI_ERR_HIP: return "HIP runtime error.";
    case AAI_ERR_EMPTY_OUTPUT: return "Output image would be empty.";
    default: return "Unknown error.";
    }
}

int aai_query(const aai_request *req, aai_layout *out)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    if (!out) return fail(AAI_ERR_BAD_ARGUMENT, "Null layout.");
    AAI_TRY(request_geometry(*req, g));
    return finish(*req, g, out);
}

int aai_device_count(int *count)
{
    if (!count) return fail(AAI_ERR_BAD_ARGUMENT, "Null count.");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
    return AAI_OK;
}

int aai_set_device(int ordinal)
{
    AAI_TRY(require_device());
    AAI_HIP(hipSetDevice(ordinal));
    return AAI_OK;
}

int aai_device_synchronize(void)
{
    AAI_TRY(require_device());
    AAI_HIP(hipDeviceSynchronize());
    return AAI_OK;
}

int aai_resample_batch_device(const aai_request *req, int32_t batch, const void *d_src, int32_t src_dtype,
                              int64_t src_stride, int64_t src_image_stride,
                              float *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_dtype(src_dtype));
    AAI_TRY(check_batch(batch));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(d_src, d_dst));
    return device_tail(false, [&] {
        return enqueue(*req, g, batch, d_src, src_dtype, src_stride, src_image_stride, d_dst, dst_stride, dst_image_stride, (hipStream_t)stream);
    });
}

int aai_resample_batch_device_f32(const aai_request *req, int32_t batch,
                                  const float *d_src, int64_t src_stride, int64_t src_image_stride,
                                  float *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream)
{
    return aai_resample_batch_device(req, batch, d_src, AAI_DTYPE_F32, src_stride, src_image_stride, d_dst, dst_stride, dst_image_stride, stream);
}

int aai_resample_batch_multi_device_f32(const aai_request *req, int32_t n_shards, const int32_t *devices, const int32_t *counts,
                                        const float *const *d_src, int64_t src_stride, int64_t src_image_stride,
                                        float *const *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *const *streams)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    if (n_shards < 0 || (n_shards > 0 && (!devices || !counts || !d_src || !d_dst))) return fail(AAI_ERR_BAD_ARGUMENT, "Bad shard description.");
    AAI_TRY(request_geometry(*req, g));
    for (int i = 0; i < n_shards; ++i) {
        AAI_TRY(check_batch(counts[i]));
        if (counts[i] > 0) AAI_TRY(check_pointers(d_src[i], d_dst[i]));
    }
    AAI_TRY(require_device());
    int home = 0, rc = AAI_OK;
    AAI_HIP(hipGetDevice(&home));
    for (int i = 0; i < n_shards && rc == AAI_OK; ++i) {
        if (counts[i] == 0) continue;
        const hipError_t e = hipSetDevice(devices[i]);
        if (e != hipSuccess) { rc = hip_fail(e, "hipSetDevice"); break; }
        rc = enqueue(*req, g, counts[i], d_src[i], aai::SRC_F32, src_stride, src_image_stride, d_dst[i], dst_stride, dst_image_stride,
                     streams ? (hipStream_t)streams[i] : nullptr);
    }
    (void)hipSetDevice(home);
    if (rc == AAI_OK) g_lastError.clear();
    return rc;
}

int aai_resample_device_f32(const aai_request *req, const float *d_src, int64_t src_stride,
                            float *d_dst, int64_t dst_stride, void *stream)
{
    return aai_resample_batch_device_f32(req, 1, d_src, src_stride, 0, d_dst, dst_stride, 0, stream);
}

int aai_band_source_rows(const aai_request *req, int32_t dst_row0, int32_t dst_row1, int32_t *src_row0, int32_t *src_row1)
{
    aai::Geometry g;
    return band_source_rows(req, dst_row0, dst_row1, src_row0, src_row1, g);
}

int aai_resample_band_device_f32(const aai_request *req, int32_t dst_row0, int32_t dst_row1,
                                 const float *d_src_rows, int64_t src_stride, float *d_dst_rows, int64_t dst_stride, void *stream)
{
    aai::Geometry g;
    int32_t a, b;
    AAI_TRY(band_source_rows(req, dst_row0, dst_row1, &a, &b, g));
    AAI_TRY(check_pointers(d_src_rows, d_dst_rows));
    return device_tail(false, [&] {
        return enqueue(*req, g, 1, d_src_rows, aai::SRC_F32, src_stride, 0, d_dst_rows, dst_stride, 0, (hipStream_t)stream, dst_row0, dst_row1);
    });
}

int aai_prepare(const aai_request *req, int32_t channels)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(request_geometry(*req, g));
    return device_tail(false, [&] {
        PlanRef p;
        // (the plan of a packed fp32 image: what the device entries build on their first call)
        return acquire_plan(*req, g, -1, -1, channels, rot_form(*req, g, channels, aai::SRC_F32, (int64_t)g.W * channels), &p);
    });
}

int aai_plan_info(const aai_request *req, int32_t channels, char *text, int32_t capacity)
{
    AAI_TRY(check_request(req));
    if (!text || capacity <= 0) return fail(AAI_ERR_BAD_ARGUMENT, "Null text buffer.");
    AAI_TRY(require_device());
    const std::string d = plan_description(*req, channels);
    snprintf(text, (size_t)capacity, "%s", d.c_str());
    g_lastError.clear();
    return AAI_OK;
}

int aai_shutdown(void)
{
    drop_plans();
    g_lastError.clear();
    return AAI_OK;
}

int aai_adjoint_batch_device_f32(const aai_request *req, int32_t batch,
                                 const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                 float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_GENERAL, false, req, batch, 1, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_f32(const aai_request *req, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout)
{
    return adjoint_host(ADJOINT_GENERAL, false, req, 1, gdst, dst_stride, gsrc, src_stride, layout);
}

int aai_resample_batch_device_f64(const aai_request *req, int32_t batch, const double *d_src, int64_t src_stride, int64_t src_image_stride,
                                  double *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_f64_forward(req, batch, d_src, src_stride, d_dst, dst_stride, g));
    return device_tail(batch == 0, [&] {
        return enqueue_f64_forward(*req, g, batch, d_src, src_stride, src_image_stride, d_dst, dst_stride, dst_image_stride, (hipStream_t)stream);
    });
}

int aai_resample_exact_f64(const aai_request *req, const double *src, int64_t src_stride, double *dst, int64_t dst_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_f64_forward(req, 1, src, src_stride, dst, dst_stride, g));
    AAI_TRY(require_device());
    const HostImage in = src_image(g, 1, src, src_stride, sizeof(double)), out = dst_image(g, 1, dst, dst_stride, sizeof(double));
    if (!out.bytes()) return finish(*req, g, layout);
    return round_trip(*req, g, in, out, true, layout, [&](const void *dSrc, void *dDst, hipStream_t stream) {
        return enqueue_f64_forward(*req, g, 1, static_cast<const double *>(dSrc), in.row, 0, static_cast<double *>(dDst), out.row, 0, stream);
    });
}

int aai_adjoint_batch_device_f64(const aai_request *req, int32_t batch, const double *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                 double *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_adjoint(ADJOINT_GENERAL, req, batch, false, 1, nullptr, d_gdst, dst_stride, d_gsrc, src_stride, g));
    return device_tail(batch == 0, [&] {
        return enqueue_f64_adjoint(*req, g, batch, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, (hipStream_t)stream);
    });
}

int aai_adjoint_f64(const aai_request *req, const double *gdst, int64_t dst_stride, double *gsrc, int64_t src_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_adjoint(ADJOINT_GENERAL, req, 1, false, 1, nullptr, gdst, dst_stride, gsrc, src_stride, g));
    AAI_TRY(require_device());
    const HostImage in = dst_image(g, 1, gdst, dst_stride, sizeof(double)), out = src_image(g, 1, gsrc, src_stride, sizeof(double));
    return round_trip(*req, g, in, out, true, layout, [&](const void *dGdst, void *dGsrc, hipStream_t stream) {
        return enqueue_f64_adjoint(*req, g, 1, static_cast<const double *>(dGdst), in.row, 0, static_cast<double *>(dGsrc), out.row, 0, stream);
    });
}

// The checks of aai_resample_batch_device_f32 in its order -- that entry reports its strides from enqueue(), behind the device check, and so
// does this one -- with the element type where aai_resample_batch_device checks its src_dtype.
int aai_resample_half_batch_device(const aai_request *req, int32_t batch, int32_t half_dtype, const void *d_src, int64_t src_stride, int64_t src_image_stride,
                                   void *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_half_dtype(half_dtype));
    AAI_TRY(check_batch(batch));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(d_src, d_dst));
    return device_tail(batch == 0, [&] { return check_strides(g, 1, src_stride, dst_stride); }, [&] {
        return enqueue_half(*req, g, batch, 1, half_dtype, d_src, src_stride, src_image_stride, d_dst, dst_stride, dst_image_stride, (hipStream_t)stream);
    });
}

// (a host entry: the checks of aai_resample_host)
int aai_resample_half_host(const aai_request *req, int32_t half_dtype, const void *src, int64_t src_stride, void *dst, int64_t dst_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_half_dtype(half_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_strides(g, 1, src_stride, dst_stride));
    AAI_TRY(require_device());
    return narrow_round_trip(*req, g, 1, sizeof(uint16_t), src, src_stride, dst, dst_stride, layout, [&](const void *dSrc, void *dDst, hipStream_t stream) {
        return enqueue_half(*req, g, 1, 1, half_dtype, dSrc, g.W, 0, dDst, g.dW, 0, stream);
    });
}

// ---- include/aai_half_interleaved.h: the checks of aai_resample_interleaved_device / _host in their order, like the integer entries
// below, with the half element type where those entries check their src_dtype
int aai_resample_half_interleaved_device(const aai_request *req, int32_t batch, int32_t channels, int32_t half_dtype, const void *d_src, int64_t src_stride,
                                         int64_t src_image_stride, void *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_batch(batch));
    AAI_TRY(check_half_dtype(half_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_row_length(g, channels));
    if (batch > 0 && g.dW > 0 && g.dH > 0) AAI_TRY(check_pointers(d_src, d_dst));
    return device_tail(batch == 0, [&] { return check_strides(g, channels, src_stride, dst_stride); }, [&] {
        return enqueue_half(*req, g, batch, channels, half_dtype, d_src, src_stride, src_image_stride, d_dst, dst_stride, dst_image_stride, (hipStream_t)stream);
    });
}

int aai_resample_half_interleaved_host(const aai_request *req, int32_t channels, int32_t half_dtype, const void *src, int64_t src_stride, void *dst,
                                       int64_t dst_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_half_dtype(half_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_row_length(g, channels));
    AAI_TRY(check_strides(g, channels, src_stride, dst_stride));
    AAI_TRY(require_device());
    return narrow_round_trip(*req, g, channels, sizeof(uint16_t), src, src_stride, dst, dst_stride, layout, [&](const void *dSrc, void *dDst, hipStream_t stream) {
        return enqueue_half(*req, g, 1, channels, half_dtype, dSrc, (int64_t)g.W * channels, 0, dDst, (int64_t)g.dW * channels, 0, stream);
    });
}

// The checks of aai_resample_interleaved_device in its order -- that entry reports its strides from enqueue(), behind the device check, and
// so does this one -- with the element type where that entry checks its src_dtype.
int aai_resample_int_batch_device(const aai_request *req, int32_t batch, int32_t channels, int32_t dtype, const void *d_src, int64_t src_stride,
                                  int64_t src_image_stride, void *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_batch(batch));
    AAI_TRY(check_int_dtype(dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_row_length(g, channels));
    if (batch > 0 && g.dW > 0 && g.dH > 0) AAI_TRY(check_pointers(d_src, d_dst));
    return device_tail(batch == 0, [&] { return check_strides(g, channels, src_stride, dst_stride); }, [&] {
        return enqueue_int(*req, g, batch, channels, dtype, d_src, src_stride, src_image_stride, d_dst, dst_stride, dst_image_stride, (hipStream_t)stream);
    });
}

// (a host entry: the checks of aai_resample_interleaved_host)
int aai_resample_int_host(const aai_request *req, int32_t channels, int32_t dtype, const void *src, int64_t src_stride, void *dst, int64_t dst_stride,
                          aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_int_dtype(dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_row_length(g, channels));
    AAI_TRY(check_strides(g, channels, src_stride, dst_stride));
    AAI_TRY(require_device());
    return narrow_round_trip(*req, g, channels, aai::src_elem_size(dtype), src, src_stride, dst, dst_stride, layout, [&](const void *dSrc, void *dDst, hipStream_t stream) {
        return enqueue_int(*req, g, 1, channels, dtype, dSrc, (int64_t)g.W * channels, 0, dDst, (int64_t)g.dW * channels, 0, stream);
    });
}

// ---- include/ext/aai_convert.h: the checks of aai_resample_interleaved_device / _host in their order, the element type where the integer
// entries check theirs, then the conversion's own.  The strides stand where the entry each is modelled on reports them: the device
// entry's behind the device check (as enqueue() reports that entry's), the host entry's in front of the conversion's checks.
static bool convert_planar(const aai_convert *cv) { return cv && cv->out_layout == AAI_LAYOUT_PLANAR; }

static int check_convert(const aai_convert *cv, int channels)
{
    if (!cv) return fail(AAI_ERR_BAD_ARGUMENT, "Null conversion.");
    if (cv->out_type != AAI_DTYPE_F32 && cv->out_type != AAI_HALF_F16 && cv->out_type != AAI_HALF_BF16) return fail(AAI_ERR_BAD_ARGUMENT, "Unknown output element type.");
    if (cv->out_layout != AAI_LAYOUT_INTERLEAVED && cv->out_layout != AAI_LAYOUT_PLANAR) return fail(AAI_ERR_BAD_ARGUMENT, "Unknown output layout.");
    for (int c = 0; c < channels; ++c)
        if (!std::isfinite(cv->scale[c]) || !std::isfinite(cv->offset[c])) return fail(AAI_ERR_NONFINITE, "Conversion scale and offset must be finite.");
    return AAI_OK;
}

// check_strides with a planar destination's rows of dst_width elements
static int check_convert_strides(const aai::Geometry &g, int channels, bool planar, int64_t srcStride, int64_t dstStride)
{
    if (!planar) return check_strides(g, channels, srcStride, dstStride);
    if (srcStride < (int64_t)g.W * channels) return fail(AAI_ERR_BAD_ARGUMENT, "Source stride smaller than the image width.");
    if (dstStride < (int64_t)g.dW) return fail(AAI_ERR_BAD_ARGUMENT, "Destination stride smaller than the output width.");
    return AAI_OK;
}

static int check_convert_plane(const aai::Geometry &g, bool planar, int64_t dstStride, int64_t planeStride)
{
    if (planar && g.dW > 0 && g.dH > 0 && planeStride < (int64_t)(g.dH - 1) * dstStride + g.dW) return fail(AAI_ERR_BAD_ARGUMENT, "Destination plane stride smaller than one plane.");
    return AAI_OK;
}

static aai::ConvertParams convert_params(const aai_convert &cv, int64_t planeStride)
{
    aai::ConvertParams p{};
    p.outType = cv.out_type == AAI_DTYPE_F32 ? aai::CONVERT_F32 : (cv.out_type == AAI_HALF_F16 ? aai::CONVERT_F16 : aai::CONVERT_BF16);
    p.planar = cv.out_layout == AAI_LAYOUT_PLANAR ? 1 : 0;
    p.planeStride = planeStride;
    for (int i = 0; i < 4; ++i) { p.scale[i] = cv.scale[i]; p.offset[i] = cv.offset[i]; }
    return p;
}

int aai_resample_convert_device(const aai_request *req, int32_t batch, int32_t channels, int32_t src_dtype, const void *d_src, int64_t src_stride,
                                int64_t src_image_stride, const aai_convert *cv, void *d_dst, int64_t dst_stride, int64_t dst_plane_stride,
                                int64_t dst_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_batch(batch));
    AAI_TRY(check_int_dtype(src_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_row_length(g, channels));
    if (batch > 0 && g.dW > 0 && g.dH > 0) AAI_TRY(check_pointers(d_src, d_dst));
    AAI_TRY(check_convert(cv, channels));
    const bool planar = convert_planar(cv);
    return device_tail(batch == 0, [&] {
        AAI_TRY(check_convert_strides(g, channels, planar, src_stride, dst_stride));
        return check_convert_plane(g, planar, dst_stride, dst_plane_stride);
    }, [&] {
        return enqueue_convert(*req, g, batch, channels, src_dtype, d_src, src_stride, src_image_stride, convert_params(*cv, dst_plane_stride), d_dst, dst_stride,
                               dst_image_stride, (hipStream_t)stream);
    });
}

// (a host entry: one image up, one enqueue on the null stream, the wait, the image down -- a planar one plane by plane -- on dense device twins)
int aai_resample_convert_host(const aai_request *req, int32_t channels, int32_t src_dtype, const void *src, int64_t src_stride, const aai_convert *cv, void *dst,
                              int64_t dst_stride, int64_t dst_plane_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_int_dtype(src_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_row_length(g, channels));
    const bool planar = convert_planar(cv);
    AAI_TRY(check_convert_strides(g, channels, planar, src_stride, dst_stride));
    AAI_TRY(check_convert(cv, channels));
    AAI_TRY(check_convert_plane(g, planar, dst_stride, dst_plane_stride));
    AAI_TRY(require_device());
    const size_t osz = cv->out_type == AAI_DTYPE_F32 ? sizeof(float) : sizeof(uint16_t);
    const HostImage in = src_image(g, channels, src, src_stride, aai::src_elem_size(src_dtype));
    // the device twin: dH rows of dW x channels elements, or `channels` planes of dH rows of dW elements
    const int64_t row = planar ? (int64_t)g.dW : (int64_t)g.dW * channels;
    const int planes = planar ? channels : 1;
    const size_t planeBytes = osz * (size_t)row * (size_t)g.dH;
    if (!planeBytes) return finish(*req, g, layout);
    DeviceBuffer dIn, dOut;
    hipStream_t stream = nullptr;
    AAI_HIP(dIn.alloc(in.bytes()));
    AAI_HIP(dOut.alloc(planeBytes * (size_t)planes));
    AAI_HIP(hipMemcpy2D(dIn.p, in.esz * in.row, in.p, in.esz * in.stride, in.esz * in.row, in.rows, hipMemcpyHostToDevice));
    AAI_TRY(enqueue_convert(*req, g, 1, channels, src_dtype, dIn.p, in.row, 0, convert_params(*cv, row * g.dH), dOut.p, row, 0, stream));
    AAI_HIP(hipStreamSynchronize(stream));
    for (int c = 0; c < planes; ++c)
        AAI_HIP(hipMemcpy2D(static_cast<char *>(dst) + osz * (size_t)c * (size_t)dst_plane_stride, osz * dst_stride, dOut.as<char>() + planeBytes * (size_t)c, osz * row,
                            osz * row, g.dH, hipMemcpyDeviceToHost));
    return finish(*req, g, layout);
}

int aai_adjoint_prepare(const aai_request *req) { return adjoint_prepare(ADJOINT_PLANNED, req); }

int aai_adjoint_planned_batch_device_f32(const aai_request *req, int32_t batch,
                                         const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                         float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_PLANNED, false, req, batch, 1, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_planned_f32(const aai_request *req, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout)
{
    return adjoint_host(ADJOINT_PLANNED, false, req, 1, gdst, dst_stride, gsrc, src_stride, layout);
}

int aai_adjoint_rotated_prepare(const aai_request *req) { return adjoint_prepare(ADJOINT_ROTATED, req); }

int aai_adjoint_rotated_batch_device_f32(const aai_request *req, int32_t batch,
                                         const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                         float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_ROTATED, false, req, batch, 1, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_rotated_f32(const aai_request *req, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout)
{
    return adjoint_host(ADJOINT_ROTATED, false, req, 1, gdst, dst_stride, gsrc, src_stride, layout);
}

int aai_adjoint_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                       const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                       float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_GENERAL, true, req, batch, channels, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_interleaved_f32(const aai_request *req, int32_t channels, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride,
                                aai_layout *layout)
{
    return adjoint_host(ADJOINT_GENERAL, true, req, channels, gdst, dst_stride, gsrc, src_stride, layout);
}

int aai_adjoint_rotated_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                               const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                               float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_ROTATED, true, req, batch, channels, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_rotated_interleaved_f32(const aai_request *req, int32_t channels, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride,
                                        aai_layout *layout)
{
    return adjoint_host(ADJOINT_ROTATED, true, req, channels, gdst, dst_stride, gsrc, src_stride, layout);
}

int aai_adjoint_planned_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                               const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                               float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_SEPARABLE, true, req, batch, channels, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_planned_interleaved_f32(const aai_request *req, int32_t channels, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride,
                                        aai_layout *layout)
{
    return adjoint_host(ADJOINT_SEPARABLE, true, req, channels, gdst, dst_stride, gsrc, src_stride, layout);
}

// ---- include/aai_adjoint_half.h: the checks of aai_adjoint_planned_interleaved_device_f32 / _f32 (check_adjoint) with the element type
// directly behind the channel count
int aai_adjoint_half_device(const aai_request *req, int32_t batch, int32_t channels, int32_t half_dtype, const void *d_gdst, int64_t dst_stride,
                            int64_t dst_image_stride, void *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_adjoint(ADJOINT_SEPARABLE, req, batch, true, channels, &half_dtype, d_gdst, dst_stride, d_gsrc, src_stride, g));
    return device_tail(batch == 0, [&] {
        return enqueue_adjoint_half(*req, g, batch, channels, half_dtype, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, (hipStream_t)stream);
    });
}

int aai_adjoint_half_host(const aai_request *req, int32_t channels, int32_t half_dtype, const void *gdst, int64_t dst_stride, void *gsrc, int64_t src_stride,
                          aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_adjoint(ADJOINT_SEPARABLE, req, 1, true, channels, &half_dtype, gdst, dst_stride, gsrc, src_stride, g));
    AAI_TRY(require_device());
    const HostImage in = dst_image(g, channels, gdst, dst_stride, sizeof(uint16_t)), out = src_image(g, channels, gsrc, src_stride, sizeof(uint16_t));
    return round_trip(*req, g, in, out, true, layout, [&](const void *dGdst, void *dGsrc, hipStream_t stream) {
        return enqueue_adjoint_half(*req, g, 1, channels, half_dtype, dGdst, in.row, 0, dGsrc, out.row, 0, stream);
    });
}

int aai_adjoint_sample_batch_device_f32(const aai_request *req, int32_t batch,
                                        const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                        float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_SAMPLE, false, req, batch, 1, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_sample_f32(const aai_request *req, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride, aai_layout *layout)
{
    return adjoint_host(ADJOINT_SAMPLE, false, req, 1, gdst, dst_stride, gsrc, src_stride, layout);
}

int aai_adjoint_sample_interleaved_device_f32(const aai_request *req, int32_t batch, int32_t channels,
                                              const float *d_gdst, int64_t dst_stride, int64_t dst_image_stride,
                                              float *d_gsrc, int64_t src_stride, int64_t src_image_stride, void *stream)
{
    return adjoint_device(ADJOINT_SAMPLE, true, req, batch, channels, d_gdst, dst_stride, dst_image_stride, d_gsrc, src_stride, src_image_stride, stream);
}

int aai_adjoint_sample_interleaved_f32(const aai_request *req, int32_t channels, const float *gdst, int64_t dst_stride, float *gsrc, int64_t src_stride,
                                       aai_layout *layout)
{
    return adjoint_host(ADJOINT_SAMPLE, true, req, channels, gdst, dst_stride, gsrc, src_stride, layout);
}

int aai_synth_rows_device_f32(float *d_dst, int32_t width, int32_t height, int32_t row0, int32_t row1, int64_t stride, uint64_t seed, void *stream)
{
    if (!d_dst || width < 0 || height < 0 || row0 < 0 || row1 < row0 || row1 > height || stride < width)
        return fail(AAI_ERR_BAD_ARGUMENT, "Bad synthetic image arguments.");
    AAI_TRY(require_device());
    AAI_HIP(aai::launch_synth_rows(d_dst, width, height, row0, row1, stride, seed, (hipStream_t)stream));
    return AAI_OK;
}

int aai_synth_device_f32(float *d_dst, int32_t width, int32_t height, int64_t stride, uint64_t seed, void *stream)
{
    if (!d_dst || width < 0 || height < 0 || stride < width) return fail(AAI_ERR_BAD_ARGUMENT, "Bad synthetic image arguments.");
    AAI_TRY(require_device());
    AAI_HIP(aai::launch_synth(d_dst, width, height, stride, seed, (hipStream_t)stream));
    return AAI_OK;
}

int aai_resample_host(const aai_request *req, const void *src, int32_t src_dtype, int64_t src_stride,
                      float *dst, int64_t dst_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_dtype(src_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_strides(g, 1, src_stride, dst_stride));
    AAI_TRY(require_device());
    return host_round_trip(*req, g, 1, src_dtype, false, src, src_stride, dst, dst_stride, layout);
}

int aai_resample_interleaved_device(const aai_request *req, int32_t batch, int32_t channels,
                                    const void *d_src, int32_t src_dtype, int64_t src_stride, int64_t src_image_stride,
                                    float *d_dst, int64_t dst_stride, int64_t dst_image_stride, void *stream)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_batch(batch));
    AAI_TRY(check_dtype(src_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_row_length(g, channels));
    if (batch > 0 && g.dW > 0 && g.dH > 0) AAI_TRY(check_pointers(d_src, d_dst));
    return device_tail(false, [&] {
        return enqueue(*req, g, batch, d_src, src_dtype, src_stride, src_image_stride, d_dst, dst_stride, dst_image_stride, (hipStream_t)stream, -1, -1, channels);
    });
}

int aai_resample_interleaved_host(const aai_request *req, int32_t channels, const void *src, int32_t src_dtype, int64_t src_stride,
                                  float *dst, int64_t dst_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_channels(channels));
    AAI_TRY(check_dtype(src_dtype));
    AAI_TRY(request_geometry(*req, g));
    AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_row_length(g, channels));
    AAI_TRY(check_strides(g, channels, src_stride, dst_stride));
    AAI_TRY(require_device());
    return host_round_trip(*req, g, channels, src_dtype, false, src, src_stride, dst, dst_stride, layout);
}

int aai_host_alloc(void **ptr, uint64_t bytes)
{
    if (!ptr) return fail(AAI_ERR_BAD_ARGUMENT, "Null pointer.");
    AAI_TRY(require_device());
    AAI_HIP(hipHostMalloc(ptr, bytes ? (size_t)bytes : 1, hipHostMallocDefault));
    g_lastError.clear();
    return AAI_OK;
}

int aai_host_free(void *ptr)
{
    if (!ptr) return AAI_OK;
    AAI_HIP(hipHostFree(ptr));
    return AAI_OK;
}

int aai_resample_batch_host(const aai_request *req, int32_t batch, const void *src, int32_t src_dtype,
                            int64_t src_stride, int64_t src_image_stride,
                            float *dst, int64_t dst_stride, int64_t dst_image_stride, aai_layout *layout)
{
    aai::Geometry g;
    AAI_TRY(check_request(req));
    AAI_TRY(check_dtype(src_dtype));
    AAI_TRY(check_batch(batch));
    AAI_TRY(request_geometry(*req, g));
    if (batch > 0) AAI_TRY(check_pointers(src, dst));
    AAI_TRY(check_strides(g, 1, src_stride, dst_stride));
    AAI_TRY(require_device());

    const size_t esz = aai::src_elem_size(src_dtype), srcRow = esz * g.W, dstRow = sizeof(float) * g.dW;      // bytes per dense row
    const size_t nDst = (size_t)g.dW * g.dH;
    if (batch > 0 && nDst) {
        std::lock_guard<std::mutex> lock(g_slotMutex);
        SlotPool &p = g_slots;
        AAI_HIP(p.reserve(srcRow * g.H, sizeof(float) * nDst));
        // Pageable buffers: the runtime's blocking copy (pinned bounce buffers, double-buffered) is its fastest path
        // and the asynchronous one much slower, so only page-locked buffers are copied asynchronously.
        const bool asyncUp = is_page_locked(src), asyncDown = is_page_locked(dst);
        // one image between the host and a slot (dense rows there).  Dense host images go as one linear copy: the 2-D path
        // copies row by row and is several times slower.
        auto copy_image = [](void *to, size_t toPitch, const void *from, size_t fromPitch, size_t rowBytes, size_t rows, hipMemcpyKind kind,
                             bool async, hipStream_t st) -> hipError_t {
            if (toPitch == rowBytes && fromPitch == rowBytes)
                return async ? hipMemcpyAsync(to, from, rowBytes * rows, kind, st) : hipMemcpy(to, from, rowBytes * rows, kind);
            return async ? hipMemcpy2DAsync(to, toPitch, from, fromPitch, rowBytes, rows, kind, st) : hipMemcpy2D(to, toPitch, from, fromPitch, rowBytes, rows, kind);
        };
        const char *srcBytes = static_cast<const char *>(src);
        hipError_t e = hipSuccess;
        int rc = AAI_OK;
        for (int b = 0; b < batch && e == hipSuccess; ++b) {
            const int s = b % kSlots;
            hipStream_t st = p.streams[s];
            // stream order protects the slot: this upload waits for the download of image b - kSlots
            const char *hSrc = srcBytes + esz * (size_t)b * src_image_stride;
            float *hDst = dst + (size_t)b * dst_image_stride;
            if (!asyncUp) e = hipStreamSynchronize(st);          // a blocking copy does not wait for the slot's stream
            if (e != hipSuccess) break;
            e = copy_image(p.dSrc[s], srcRow, hSrc, esz * src_stride, srcRow, g.H, hipMemcpyHostToDevice, asyncUp, st);
            if (e != hipSuccess) break;
            rc = enqueue(*req, g, 1, p.dSrc[s], src_dtype, g.W, 0, p.dDst[s], g.dW, 0, st);
            if (rc != AAI_OK) break;
            if (!asyncDown) e = hipStreamSynchronize(st);
            if (e != hipSuccess) break;
            e = copy_image(hDst, sizeof(float) * dst_stride, p.dDst[s], dstRow, dstRow, g.dH, hipMemcpyDeviceToHost, asyncDown, st);
        }
        for (int s = 0; s < kSlots; ++s) {
            const hipError_t e2 = hipStreamSynchronize(p.streams[s]);
            if (e == hipSuccess) e = e2;
        }
        if (rc != AAI_OK) return rc;
        if (e != hipSuccess) return hip_fail(e, "aai_resample_batch_host");
    }
    return finish(*req, g, layout);
}

int aai_resample_f32(const aai_request *req, const float *src, int64_t src_stride, float *dst, int64_t dst_stride, aai_layout *layout)
{
    return resample_host_plain(req, false, src, src_stride, dst, dst_stride, layout);
}

int aai_resample_f64(const aai_request *req, const double *src, int64_t src_stride, double *dst, int64_t dst_stride, aai_layout *layout)
{
    return resample_host_plain(req, true, src, src_stride, dst, dst_stride, layout);
}

}  // extern "C"
