"""ls_hit_attributes and ls_apply_return_model between frames in flight: their place in the handle's stream order when they run on
a caller stream (the hand-over every query entry point shares, query_enter / query_leave)."""
import numpy as np
import pytest

from conftest import make_tracer
from test_gpu_attr import _ground_ben

pytestmark = pytest.mark.gpu


def test_frames_around_attributes_and_returns_on_a_caller_stream(oracle, capi, sensors, meshes):
    """LS_OPT_PIPELINE = 2, three frames in flight: ls_hit_attributes and ls_apply_return_model (the identity model; once with n = 0)
    on a caller stream over the device hit records of one of those frames, a pose change, a frame again -- every frame the oracle's
    cloud, the attributes and returns those of the same calls on the handle's stream after a full synchronise"""
    import torch
    s = sensors["0000"]
    n = s.V * s.H
    tr = make_tracer(capi, s, "projection")
    tr.setOption(capi.LS_OPT_PIPELINE, 2)
    ml = _ground_ben(tr, oracle, meshes)
    A_new = oracle.affine_from_components(np.float32([0.4, -0.3, 0.1]), np.float32([0.0, 0.0, 0.5]))
    refs = [oracle.trace_frame(s, ml), oracle.trace_frame(s, [ml[0], (1, *meshes["ben"], A_new)])]
    assert not np.array_equal(refs[0]["points"], refs[1]["points"])
    model = capi.ReturnModel()
    frames = [(torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"),
               torch.zeros(4, dtype=torch.int32, device="cuda:0")) for _ in range(4)]

    def outputs():   # attribute records; the returns' points, hit records and count; the count of the n = 0 call
        return (torch.full((48 * n,), 0xAB, dtype=torch.uint8, device="cuda:0"), torch.full((32 * n,), 0xAB, dtype=torch.uint8, device="cuda:0"),
                torch.full((16 * n,), 0xAB, dtype=torch.uint8, device="cuda:0"), torch.full((4,), -1, dtype=torch.int32, device="cuda:0"),
                torch.full((4,), -1, dtype=torch.int32, device="cuda:0"))

    def queries(h, c, o, stream):
        assert tr.hitAttributesDevice(h.data_ptr(), n, o[0].data_ptr(), d_count=c.data_ptr(), stream=stream) == 0
        assert tr.applyReturnModelDevice(model, h.data_ptr(), n, o[3].data_ptr(), d_points32=o[1].data_ptr(), d_hits_out=o[2].data_ptr(),
                                         d_count=c.data_ptr(), stream=stream) == 0
        assert tr.applyReturnModelDevice(model, h.data_ptr(), 0, o[4].data_ptr(), stream=stream) == 0

    # what the calls give on the handle's stream, over the records of a finished frame
    want, got = outputs(), outputs()
    p, h, c = frames[1]
    torch.cuda.synchronize()
    tr.setOutputBuffers(p.data_ptr(), h.data_ptr(), c.data_ptr(), n)
    tr.traceSceneAsync(0)
    tr.flush()
    tr.synchronize()
    queries(h, c, want, None)
    tr.synchronize()
    for b in frames[1]:
        b.zero_()   # (a query that ran ahead of its frame would read no record)
    torch.cuda.synchronize()
    qs = torch.cuda.Stream()
    for i in range(3):
        tr.setOutputBuffers(*[b.data_ptr() for b in frames[i]], n)
        tr.traceSceneAsync(i)
    queries(h, c, got, qs.cuda_stream)
    tr.updateGeometryTransform("face", A_new)
    assert tr.commitScene() == 0
    tr.setOutputBuffers(*[b.data_ptr() for b in frames[3]], n)
    tr.traceSceneAsync(3)
    tr.flush()
    tr.synchronize()
    torch.cuda.synchronize()
    for i, (p, h, c) in enumerate(frames):
        ref = refs[i // 3]
        k = int(c[0].item())
        assert k == len(ref["points"]) and np.array_equal(p.cpu().numpy()[:32 * k].reshape(k, 32), ref["points"]), i
    k = len(refs[0]["points"])
    assert int(want[3][0].item()) == k and int(want[4][0].item()) == 0   # the identity model keeps every hit; n = 0: a zero count
    a = want[0].cpu().numpy()
    assert np.all(a[:48 * k].view(np.uint32).reshape(k, 12)[:, 7] == 1) and np.all(a[48 * k:] == 0xAB)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w.cpu().numpy())
    assert tr.info(capi.LS_INFO_DEVICE_STATUS) == 0
    tr.close()
