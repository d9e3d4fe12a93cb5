"""Strided host buffers on the typed host entries: what the host round trip (csrc/aai_capi.cpp) owes a caller whose rows are longer
than the image.

Every host entry uploads the caller's strided rows into dense device images, enqueues once and downloads into the caller's strided
rows.  Each entry below is called through ctypes with row strides of (dense row + 5) elements on both buffers, every byte outside the
images 0xA5.  Its result is the matching device entry's on the same data bit for bit -- the device entry runs on torch buffers and
never passes through the round trip -- and the padding of the output still holds 0xA5.  (Padding of the input that was read would
change the bits: 0xA5... is an ordinary finite value in every element type here.)

One request at 0 degrees (the direct routes of the narrow-element entries) and one at 17.5 (their forwarding routes), 2:1
down-sampling of a 37 x 23 source, three channels where the entry is interleaved.

And the one check of the entry layer that sits behind the device check, which the recording of tests/test_entry_point_errors.py cannot
see: the strides of the half / integer device entries.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, PAD, FILL = 37, 23, 5, 0xA5


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return aai


def _random(rng, dtype, shape):
    if dtype == np.uint8:
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    if dtype == np.uint16:                                                  # raw fp16 bits
        return rng.random(shape).astype(np.float16).view(np.uint16)
    return rng.random(shape).astype(dtype)


# name -> (element type, channels, adjoint?, host call, device call); both calls take (lib, rq, C, in, in stride, out, out stride).
# The adjoint entries name the image they read gdst and pass it first, like the forward entries their source.
def _cases(L):
    return {
        "aai_resample_exact_f64": (np.float64, 1, False,
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_exact_f64(rq, i, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_batch_device_f64(rq, 1, i, si, 0, o, so, 0, None)),
        "aai_adjoint_f64": (np.float64, 1, True,
            lambda lib, rq, C, i, si, o, so: lib.aai_adjoint_f64(rq, i, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_adjoint_batch_device_f64(rq, 1, i, si, 0, o, so, 0, None)),
        "aai_resample_half_host": (np.uint16, 1, False,
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_half_host(rq, L.HALF_F16, i, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_half_batch_device(rq, 1, L.HALF_F16, i, si, 0, o, so, 0, None)),
        "aai_resample_half_interleaved_host": (np.uint16, 3, False,
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_half_interleaved_host(rq, C, L.HALF_F16, i, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_half_interleaved_device(rq, 1, C, L.HALF_F16, i, si, 0, o, so, 0, None)),
        "aai_resample_int_host": (np.uint8, 3, False,
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_int_host(rq, C, L.DTYPE_U8, i, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_int_batch_device(rq, 1, C, L.DTYPE_U8, i, si, 0, o, so, 0, None)),
        "aai_adjoint_half_host": (np.uint16, 3, True,
            lambda lib, rq, C, i, si, o, so: lib.aai_adjoint_half_host(rq, C, L.HALF_F16, i, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_adjoint_half_device(rq, 1, C, L.HALF_F16, i, si, 0, o, so, 0, None)),
        "aai_adjoint_f32": (np.float32, 1, True,
            lambda lib, rq, C, i, si, o, so: lib.aai_adjoint_f32(rq, i, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_adjoint_batch_device_f32(rq, 1, i, si, 0, o, so, 0, None)),
        "aai_resample_interleaved_host": (np.float32, 3, False,
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_interleaved_host(rq, C, i, L.DTYPE_F32, si, o, so, None),
            lambda lib, rq, C, i, si, o, so: lib.aai_resample_interleaved_device(rq, 1, C, i, L.DTYPE_F32, si, 0, o, so, 0, None)),
    }


@pytest.mark.parametrize("entry", ["aai_resample_half_batch_device", "aai_resample_half_interleaved_device", "aai_resample_int_batch_device"])
def test_narrow_device_entry_reports_a_short_source_stride(gpu, entry):
    """The half / integer device entries check their strides behind the device check, where the recording of
    tests/test_entry_point_errors.py (made without a device) cannot see it: AAI_ERR_BAD_ARGUMENT with the stride text, before any
    launch.  (The buffers are real and large enough for the call: nothing depends on the check for its memory safety.)"""
    import torch
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    C = 1 if entry == "aai_resample_half_batch_device" else 3
    rq = gpu.make_request(W, H, 2.0, 1.0, ((W - 1) / 2.0, (H - 1) / 2.0), 0.0)
    lay = gpu.query(rq)[2]
    esz, dt = (1, L.DTYPE_U8) if entry == "aai_resample_int_batch_device" else (2, L.HALF_F16)
    src = torch.zeros(H * W * C * esz, dtype=torch.uint8, device="cuda")
    dst = torch.full((lay.dst_height * lay.dst_width * C * esz,), FILL, dtype=torch.uint8, device="cuda")
    lead = (1, dt) if C == 1 else (1, C, dt)
    rc = getattr(lib, entry)(ctypes.byref(rq), *lead, src.data_ptr(), W * C - 1, 0, dst.data_ptr(), lay.dst_width * C, 0, None)
    assert (rc, lib.aai_last_error()) == (L.ERR_BAD_ARGUMENT, b"Source stride smaller than the image width.")
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())


ENTRIES = ["aai_resample_exact_f64", "aai_adjoint_f64", "aai_resample_half_host", "aai_resample_half_interleaved_host", "aai_resample_int_host",
           "aai_adjoint_half_host", "aai_adjoint_f32", "aai_resample_interleaved_host"]


@pytest.mark.parametrize("angle", [0.0, 17.5])
@pytest.mark.parametrize("entry", ENTRIES)
def test_strided_host_call_has_the_device_entrys_bits(gpu, entry, angle):
    import torch
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    dtype, C, adjoint, host, device = _cases(L)[entry]
    rq = gpu.make_request(W, H, 2.0, 1.0, ((W - 1) / 2.0, (H - 1) / 2.0), angle)
    rc, msg, lay = gpu.query(rq)
    assert rc == L.OK and lay.dst_width > 1 and lay.dst_height > 1, msg
    src_shape, dst_shape = (H, W * C), (lay.dst_height, lay.dst_width * C)
    (rows_in, row_in), (rows_out, row_out) = (dst_shape, src_shape) if adjoint else (src_shape, dst_shape)
    esz = np.dtype(dtype).itemsize

    data = _random(np.random.default_rng(len(entry)), dtype, (rows_in, row_in))
    h_in = np.full((rows_in, (row_in + PAD) * esz), FILL, np.uint8).view(dtype)
    h_in[:, :row_in] = data
    h_out = np.full((rows_out, (row_out + PAD) * esz), FILL, np.uint8).view(dtype)
    given = h_in.copy()
    assert host(lib, ctypes.byref(rq), C, h_in.ctypes.data, row_in + PAD, h_out.ctypes.data, row_out + PAD) == L.OK, lib.aai_last_error()
    host_kernel = gpu.last_kernel()

    d_in = torch.from_numpy(data.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.full((rows_out * row_out * esz,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert device(lib, ctypes.byref(rq), C, d_in.data_ptr(), row_in, d_out.data_ptr(), row_out) == L.OK, lib.aai_last_error()
    torch.cuda.synchronize()
    want = d_out.cpu().numpy().view(dtype).reshape(rows_out, row_out)

    assert gpu.last_kernel() == host_kernel, (host_kernel, gpu.last_kernel())
    assert (h_out[:, row_out:].view(np.uint8) == FILL).all(), (entry, angle, host_kernel, "the padding of the output rows was written")
    assert np.array_equal(h_in.view(np.uint8), given.view(np.uint8)), (entry, angle, "the input was written")
    differ = h_out[:, :row_out].view(np.uint8) != want.view(np.uint8)
    assert not differ.any(), (entry, angle, host_kernel, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    assert (want.view(np.uint8) != FILL).any()                              # (the device entry wrote something: the comparison is of results)
