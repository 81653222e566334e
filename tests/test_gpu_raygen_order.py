"""ls_generate_rays / ls_generate_rays_aos write into buffers the caller has just made: the kernel is ordered behind what the device's
default stream held when the call was made, so a fill of the new buffer that is still queued there cannot land on top of the rays."""
import numpy as np
import pytest

from conftest import make_tracer

pytestmark = pytest.mark.gpu


def test_ray_generators_wait_for_the_default_stream(capi, sensors):
    """8 GiB of fills queued on the default stream (milliseconds of work), then the zero-fill of the new ray buffer, then the call with
    no synchronize in between: the rays are the ones a call on a settled device writes, not zeros"""
    import torch
    s = sensors["0000"]
    tr = make_tracer(capi, s)
    n = tr.getTotalRays()
    assert n == 4800
    want = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    soa_want = torch.zeros(3 * n, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    tr.generateRaysAos(want.data_ptr(), None)
    tr.generateRays(soa_want[:n].data_ptr(), soa_want[n:2 * n].data_ptr(), soa_want[2 * n:].data_ptr())
    tr.synchronize()
    want, soa_want = want.cpu().numpy(), soa_want.cpu().numpy()
    d = want.view(np.float32).reshape(n, 8)[:, 4:7]
    assert np.all(np.any(d != 0, axis=1)) and np.array_equal(d.T.reshape(-1), soa_want)
    big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(3):
        for _ in range(8):
            big.zero_()
        rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
        soa = torch.zeros(3 * n, dtype=torch.float32, device="cuda:0")
        tr.generateRaysAos(rays.data_ptr(), None)
        tr.generateRays(soa[:n].data_ptr(), soa[n:2 * n].data_ptr(), soa[2 * n:].data_ptr())
        tr.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(rays.cpu().numpy(), want)
        assert np.array_equal(soa.cpu().numpy(), soa_want)
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
