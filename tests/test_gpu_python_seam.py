"""The Python wrappers on the device seam: every single defect of tests/seam_cases.py on CUDA tensors is refused with the exception
class and the whole message it always had, before any kernel runs, and leaves every argument as it was; and a call inside
torch.cuda.stream(s) runs on s -- the device is set first and its current stream read then -- and gives the host seam's bits."""
import numpy as np
import pytest

import seam_cases as C

pytestmark = pytest.mark.gpu

DEVICE_WRAPPERS = [w for w in C.WRAPPERS if w.device]


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


def _refused(lsf, w, kw, exc, msg):
    before = C.freeze(kw)
    with pytest.raises(exc) as e:
        getattr(lsf, w.name)(**kw)
    assert type(e.value) is exc and str(e.value) == msg
    assert C.freeze(kw) == before


@pytest.mark.parametrize("w", DEVICE_WRAPPERS, ids=[w.name for w in DEVICE_WRAPPERS])
def test_a_single_defect_on_the_device_seam_is_refused_with_the_message_it_always_had(lsf, w):
    cases = C.device_defects(w)
    assert len(cases) >= 3
    for did, patch, exc, msg in cases:
        print(w.name, did)
        _refused(lsf, w, C.apply(w.valid(C.Make("cuda")), patch), exc, msg)


@pytest.mark.parametrize("w", [w for w in DEVICE_WRAPPERS if len(w.fields) + len(w.points) > 1], ids=lambda w: w.name)
def test_a_tensor_among_numpy_arrays_is_refused(lsf, w):
    import torch

    other = next(f for f in w.fields + w.points if f.path != w.anchor)
    kw = w.valid(C.Make("np"))
    a = C.get(kw, other.path)
    C.put(kw, other.path, torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda"))
    _refused(lsf, w, kw, TypeError, w.kind_msg or f"{other.name} must be a numpy array of {other.dtype}")


@pytest.mark.parametrize("w", [w for w in DEVICE_WRAPPERS if w.one_device_msg], ids=lambda w: w.name)
def test_tensors_on_two_devices_are_refused(lsf, w):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    other = next(f for f in w.fields + w.points if f.path != w.anchor)
    kw = w.valid(C.Make("cuda"))
    a = C.get(kw, other.path)
    C.put(kw, other.path, a.t().contiguous().to("cuda:1").t() if a.dim() == 2 else a.to("cuda:1"))
    _refused(lsf, w, kw, ValueError, w.one_device_msg)


def test_the_table_puts_a_host_tensor_among_device_tensors():
    ids = {f"{w.name}-{did}" for w in DEVICE_WRAPPERS for did, *_ in C.device_defects(w)}
    for want in ("advectPoints-pts-on-the-host", "advectPoints-u-on-the-host", "correctField-pts-on-the-host", "correctField-mask-on-the-host",
                 "reseedParticles-pts-on-the-host", "samplePoints-pts-on-the-host", "extendField-phi-on-the-host", "narrowBand-phiNB-on-the-host",
                 "correctField-pts-missing", "correctField-rad-missing", "samplePoints-pts-missing", "castRays-dir-missing",
                 "extendField-phi-missing"):
        assert want in ids, want


def test_a_stacked_velocity_is_three_fields(lsf):
    """advectPoints takes the velocity's three entries, whatever holds them: torch.stack((u, v, w)) gives the tuple's result"""
    import torch

    w = next(w for w in C.WRAPPERS if w.name == "advectPoints")
    kw = w.valid(C.Make("cuda"))
    want, got = lsf.advectPoints(**kw), lsf.advectPoints(**dict(kw, velocity=torch.stack(kw["velocity"])))
    torch.cuda.synchronize()
    assert torch.equal(got.pts, want.pts) and torch.equal(got.status, want.status) and got.info == want.info
    assert sum(want.info[:4]) == 3  # the call ran: every point has one of the four statuses


def test_a_call_runs_on_the_tensors_current_stream(lsf):
    import torch

    host, dev = C.Make("np"), C.Make("cuda")
    nb, sb = host.i32(-7), host.i32(-7)
    lsf.narrowBand(*C.N, C.DX, host.f64(), nb, sb)
    ref = lsf.samplePoints(host.f64(), *C.N, C.DX, C.LO, host.pts(), q=host.f64(2.0), iso=0.05, iters=2)
    assert 0 < int(nb.sum()) < nb.size and int(ref.info[0]) >= 1  # the band holds some cells and not all, a point was sampled

    phi, tnb, tsb, pts, q = dev.f64(), dev.i32(-7), dev.i32(-7), dev.pts(), dev.f64(2.0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(s):
        lsf.narrowBand(*C.N, C.DX, phi, tnb, tsb)
        got = lsf.samplePoints(phi, *C.N, C.DX, C.LO, pts, q=q, iso=0.05, iters=2)
    s.synchronize()
    assert np.array_equal(tnb.cpu().numpy().T, nb) and np.array_equal(tsb.cpu().numpy().T, sb)
    for name in ("val", "grad", "qval", "foot", "status"):
        a, b = getattr(got, name).cpu().numpy(), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name
    assert got.info == ref.info
