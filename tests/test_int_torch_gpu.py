"""resample(..., integer=True) on the MI355X: uint8 / uint16 tensors in, the same dtype out (include/aai_int.h) -- the three shapes, the
zero-copy channels_last route, contiguous NCHW as single-channel images, and what the operator refuses."""
import numpy as np
import pytest

import int_cases as ic

pytestmark = pytest.mark.gpu

GEOM = ic.GEOMETRIES["d"]            # 67 outputs in a strip: on the direct route for both types
ARGS = GEOM[2:]


@pytest.fixture(scope="module")
def gpu(aai):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    aai.set_device(0)
    return aai


def dtypes():
    import torch
    return [(torch.uint8, ic.U8)] + ([(torch.uint16, ic.U16)] if hasattr(torch, "uint16") else [])


def images(shape, dt, seed):
    """a device tensor of `shape` with random elements over the full range of the type, and its host copy"""
    import torch
    host = np.random.default_rng(seed).integers(0, ic.MAXV[dt] + 1, size=shape).astype(ic.NP[dt])
    bits = torch.from_numpy(host.view(np.uint8).copy()).cuda()
    return (bits if dt == ic.U8 else bits.view(torch.uint16)).view(shape), host


def host(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint8 if t.dtype == torch.uint8 else np.uint16).reshape(tuple(t.shape))


def c_abi(gpu, dt, img):
    """one [H, W, C] host image through resample_int_device -> [dH, dW, C]"""
    import torch
    H, W, C = img.shape
    rq = ic.request(gpu, GEOM, "area")
    lay = gpu.query(rq)[2]
    x = torch.from_numpy(np.ascontiguousarray(img).view(np.uint8).reshape(-1).copy()).cuda()
    y = torch.zeros(lay.dst_height * lay.dst_width * C * img.itemsize, dtype=torch.uint8, device="cuda")
    gpu.resample_int_device(rq, C, x.data_ptr(), W * C, y.data_ptr(), lay.dst_width * C, dt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(img.dtype).reshape(lay.dst_height, lay.dst_width, C)


def test_each_shape_keeps_the_dtype_and_has_the_c_abis_bits(gpu):
    import torch
    W, H = GEOM[:2]
    for tdt, dt in dtypes():
        for shape in ((H, W), (2, H, W), (2, 3, H, W)):
            x, xh = images(shape, dt, 3)
            y, iso = gpu.resample(x, *ARGS, integer=True)
            assert gpu.last_kernel() == "aai_axis_int_kernel<%s>" % ("u8" if dt == ic.U8 else "u16")
            assert y.dtype == tdt and y.is_contiguous() and not y.requires_grad and tuple(y.shape[:-2]) == shape[:-2]
            planes_in, planes_out = xh.reshape(-1, H, W), host(y).reshape((-1,) + tuple(y.shape[-2:]))
            for p in range(planes_in.shape[0]):
                assert np.array_equal(planes_out[p], c_abi(gpu, dt, planes_in[p][:, :, None])[:, :, 0]), (shape, p)


def test_channels_last_is_read_in_place_and_nchw_runs_plane_by_plane(gpu):
    import torch
    W, H = GEOM[:2]
    for tdt, dt in dtypes():
        x, xh = images((2, H, W, 3), dt, 4)              # NHWC storage
        xcl = x.permute(0, 3, 1, 2)                      # (B, C, H, W), dense in channels_last
        assert xcl.is_contiguous(memory_format=torch.channels_last) and not xcl.is_contiguous()
        y, _ = gpu.resample(xcl, *ARGS, integer=True)
        assert y.dtype == tdt and y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
        assert "flagged=0" in gpu.plan_shape(ic.request(gpu, GEOM, "area"), 3)        # the 3-channel plan exists: the tensor was not split
        yh = host(y.permute(0, 2, 3, 1))
        for b in range(2):
            assert np.array_equal(yh[b], c_abi(gpu, dt, xh[b])), b
        # contiguous NCHW, C = 3: three single-channel calls per image
        xn = xcl.contiguous()
        yn, _ = gpu.resample(xn, *ARGS, integer=True)
        assert yn.is_contiguous() and yn.dtype == tdt
        ynh = host(yn)
        for b in range(2):
            for c in range(3):
                assert np.array_equal(ynh[b, c], c_abi(gpu, dt, xh[b][:, :, c:c + 1])[:, :, 0]), (b, c)
        # (the two routes sum in the same order per element: the same bits)
        assert np.array_equal(ynh, host(y))


def test_what_the_operator_refuses(gpu):
    import torch
    W, H = GEOM[:2]
    x, _ = images((H, W), ic.U8, 5)
    for extra in ({"half": True}, {"f64": True}, {"planned_backward": True}, {"planned_backward": "any"}, {"sampler_backward": True}):
        with pytest.raises(ValueError):
            gpu.resample(x, *ARGS, integer=True, **extra)
    with pytest.raises(TypeError):
        gpu.resample(torch.zeros((H, W), dtype=torch.float32, device="cuda"), *ARGS, integer=True)
    with pytest.raises(TypeError):
        gpu.resample(torch.zeros((H, W), dtype=torch.int16, device="cuda"), *ARGS, integer=True)
    with pytest.raises(TypeError) as e:
        gpu.resample(x, *ARGS)                            # without integer=True: as before
    assert "float32" in str(e.value)
    with pytest.raises(ValueError):
        gpu.resample(torch.zeros((1, 5, H, W), dtype=torch.uint8, device="cuda"), *ARGS, integer=True)
    y, _ = gpu.resample(torch.zeros((0, H, W), dtype=torch.uint8, device="cuda"), *ARGS, integer=True)
    assert y.shape[0] == 0 and y.dtype == torch.uint8
