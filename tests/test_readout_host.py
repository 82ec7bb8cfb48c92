"""
The read-out reference (tests/readout_ref.py) against hand-worked three-cell examples, and the Python read-out of the batched file route,
JobRunner._normalise, against that reference on CPU tensors: it is a staticmethod and knows no device.  No GPU.
tests/test_gpu_readout.py holds the C read-outs and _normalise on the device to the same reference.
"""

import types

import numpy as np
import pytest

from tests import readout_ref as ref

F32 = np.float32


def test_amplitudes():
    assert ref.amplitude('solar', direct_top=0.75) == 0.75
    assert ref.amplitude('thermal', src_flx=2.0, ptot=600.0, lx=10.0, ly=20.0) == 6.0
    assert ref.amplitude('solar+thermal', src_flx=2.0, ptot=600.0, psol=200.0, lx=10.0, ly=20.0) == 8.0
    assert ref.solar_amplitude(2.0, 180.0) == 2.0 and abs(ref.solar_amplitude(1.0, 120.0)-0.5) < 1e-15
    with pytest.raises(ValueError):
        ref.amplitude('local')


def test_three_cells_by_hand():
    # radiance: 2 x 2 pixels of a satellite view, 8 photons, amplitude 1/2: one unit of tally is 1/2 x 4 / 8 = 1/4
    r = ref.radiance([0.0, 1.0, 3.0], 0.5, 'satellite', 8, nxr=2, nyr=2)
    assert r.dtype == F32 and np.array_equal(r, [0.0, 0.25, 0.75])
    # a camera: 1/2 x (10 x 20) / 8 = 12.5
    assert np.array_equal(ref.radiance([0.0, 1.0, 3.0], 0.5, 'camera', 8, lx=10.0, ly=20.0), [0.0, 12.5, 37.5])
    # flux: one column, one level; raw direct 2, diffuse 6, up 10; 4 photons, amplitude 1/2: a unit is 1/8; the known direct beam 1/4
    raw = np.array([2.0, 6.0, 10.0]).reshape(3, 1, 1, 1)
    f = ref.flux(raw, 0.5, [0.25], 4)
    assert f.dtype == F32 and np.array_equal(f.ravel(), [0.5, 1.25, 1.25])          # direct; direct + diffuse (+ 1/4 each); up untouched
    assert np.array_equal(ref.flux(raw, 0.5, None, 4).ravel(), [0.25, 1.0, 1.25])
    # heating: three layers 1, 2, 4 m thick, weight 8 in each
    h = ref.heating(np.full((3, 1, 1), 8.0), 0.5, [1.0, 2.0, 4.0], 4)
    assert h.dtype == F32 and np.array_equal(h.ravel(), [1.0, 0.5, 0.25])
    A, net = ref.net_heating(np.full((3, 1, 1), 8.0), 0.5, [1.0, 2.0, 4.0], np.full((3, 1, 1), 0.5, dtype=F32), 4)
    assert np.array_equal(A.ravel(), [1.0, 0.5, 0.25]) and np.array_equal(net.ravel(), [0.5, 0.0, -0.25])


def test_run_field_and_run_statistics_by_hand():
    # two jobs into one run: float32(t norm + a) f, summed in float32
    t1, t2 = np.array([4.0, 8.0, 0.0]), np.array([2.0, 2.0, 2.0])
    run = ref.run_field([(t1, 0.25, 0.0, F32(2.0)), (t2, 0.5, np.array([1.0, 0.0, 0.0]), np.array([1.0, 3.0, 0.5], dtype=F32))])
    assert run.dtype == F32 and np.array_equal(run, [4.0, 7.0, 0.5])
    # the product and the sum round to float32, each once: 1 + 2^-24 is lost in float32, kept by a float64 sum
    tiny = ref.run_field([(np.array([1.0]), 1.0, 0.0, F32(1.0)), (np.array([2.0**-24]), 1.0, 0.0, F32(1.0))])
    assert tiny[0] == F32(1.0)
    # ... and float32(t norm + a) rounds before the factor is applied: (1 + 2^-24) x 3 is 3 in the run field, 3 (1 + 2^-24) -> 3.0000002 if not
    assert ref.run_field([(np.array([1.0+2.0**-24]), 1.0, 0.0, F32(3.0))])[0] == F32(3.0)
    t, a = ref.flux_terms(np.array([2.0, 6.0, 10.0]).reshape(3, 1, 1, 1), [0.25], share=0.0)
    assert np.array_equal(t.ravel(), [2.0, 8.0, 10.0]) and np.all(a == 0.0)
    t, a = ref.flux_terms(np.array([2.0, 6.0, 10.0]).reshape(3, 1, 1, 1), [0.25], share=1.0)
    assert np.array_equal(a.ravel(), [0.25, 0.25, 0.0])
    mean, sdev = ref.run_stats([np.array([1.0, 2.0, 3.0], dtype=F32), np.array([3.0, 2.0, 7.0], dtype=F32)])
    assert np.array_equal(mean, [2.0, 2.0, 5.0]) and np.array_equal(sdev, [1.0, 0.0, 2.0])
    assert np.array_equal(ref.ulps32(F32([1.0, -1.0, 0.0]), [np.nextafter(F32(1.0), F32(2.0)), F32(-1.0), F32(-0.0)]), [1, 0, 0])


def test_the_probes_sit_on_the_rounding_and_catch_a_float32_intermediate():
    m, f = ref.probes(4096, 3)
    up = np.nextafter(f, F32(np.inf))
    assert np.array_equal(np.nextafter(m, np.inf).astype(F32), up) and np.array_equal(np.nextafter(m, -np.inf).astype(F32), f)
    norm = ref.radiance_norm(1.4722431864335457, 'satellite', 1000003, 7, 5)
    t = m/norm
    want = ref.radiance(t, 1.4722431864335457, 'satellite', 1000003, 7, 5)
    assert np.all((want == f) | (want == up))
    single = t.astype(F32)*F32(norm)                                  # the product formed in float32
    fused_order = (t*1.4722431864335457*(35.0/1000003.0)).astype(F32)   # the factors in another order
    assert np.count_nonzero(single != want) > 1000 and np.count_nonzero(fused_order != want) > 200


# ---- JobRunner._normalise on CPU tensors -------------------------------------------------------------------------------------------------

def _meta(sc, amp, n, direct=None, rdir=None, rad_kind=2, lx=1250.0, ly=990.0, dz=None):
    return dict(scene=sc, nphoton=n, direct=direct, rdir=rdir, norm=dict(amp=amp, rad_kind=rad_kind, lx=lx, ly=ly, dz=dz))


def _tallies(n, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0.0, 1.0], 10.0**rng.uniform(-30.0, 10.0, n-2)])


@pytest.mark.parametrize('rad_kind', [2, 1])
def test_normalise_radiance_on_the_host(rad_kind):
    torch = pytest.importorskip('torch')
    from er3t_amd.rtm.mca.mca_exe import JobRunner
    sc = types.SimpleNamespace(nview=3, nyr=5, nxr=7, nz=9, ny=3, nx=5)
    amp, n = 1.4722431864335457, 1000003
    t = _tallies(105, 1)
    t[2:] = (ref.probes(103, 4)[0]/ref.radiance_norm(amp, 'camera' if rad_kind == 1 else 'satellite', n, 7, 5, 1250.0, 990.0))
    rdir = np.arange(105.0).reshape(3, 5, 7)/7.0 if rad_kind == 1 else None
    out = JobRunner._normalise(torch.from_numpy(t), (105, 0, 0), _meta(sc, amp, n, rdir=rdir, rad_kind=rad_kind))
    want = ref.radiance(t.reshape(3, 5, 7), amp, 'camera' if rad_kind == 1 else 'satellite', n, 7, 5, 1250.0, 990.0)
    assert out['rad'].dtype == torch.float32 and np.array_equal(out['rad'].numpy().view(np.uint32), want.view(np.uint32))
    assert ('rdir' in out) == (rad_kind == 1)
    if rad_kind == 1:
        assert np.array_equal(out['rdir'].numpy(), rdir.astype(F32))


@pytest.mark.parametrize('source', ['solar', 'thermal'])
def test_normalise_flux_and_heating_on_the_host(source):
    torch = pytest.importorskip('torch')
    from er3t_amd.rtm.mca.mca_exe import JobRunner
    sc = types.SimpleNamespace(nview=0, nyr=1, nxr=1, nz=9, ny=3, nx=5)
    n = 1000003
    zgrd = np.array([0.0, 137.3, 300.0, 512.5, 700.1, 1000.0, 1450.0, 2100.7, 3500.0, 6000.0])
    dz = np.diff(zgrd)
    if source == 'solar':
        amp = 1.4722431864335457
        direct = np.concatenate([np.zeros(6), amp*np.exp(-np.array([0.3, 0.2, 0.1, 0.0]))])
        sizes = (0, 450, 135)                                          # flux and heating rates (Flx_mhrt = 1)
    else:
        amp = ref.amplitude('thermal', src_flx=1.7, ptot=2.7e7, lx=1250.0, ly=990.0)        # 26 times the solar one
        direct = np.zeros(10)
        sizes = (0, 450, 0)
    t = _tallies(sum(sizes), 2)
    row = torch.from_numpy(t.copy())
    out = JobRunner._normalise(row, sizes, _meta(sc, amp, n, direct=direct, dz=dz))
    assert np.array_equal(row.numpy(), t)                              # the row is left as it was
    raw = t[:450].reshape(3, 10, 3, 5)
    want = ref.flux(raw, amp, direct, n)
    assert out['flux'].dtype == torch.float32 and np.array_equal(out['flux'].numpy().view(np.uint32), want.view(np.uint32))
    # the planes: total-down holds the direct tally, the analytic term is on the first two planes only
    f = out['flux'].numpy().astype(np.float64)
    k = ref.field_norm(amp, n, 5, 3)
    assert np.array_equal(f[2], (raw[2]*k).astype(F32)) and np.array_equal(f[1], ((raw[0]+raw[1])*k+direct[:, None, None]).astype(F32))
    if sizes[2]:
        wh = ref.heating(t[450:].reshape(9, 3, 5), amp, dz, n)
        assert np.array_equal(out['heat'].numpy().view(np.uint32), wh.view(np.uint32))
    else:
        assert 'heat' not in out


def test_source_amplitude_takes_the_thermal_power_from_the_handle():
    from er3t_amd.rtm.mca.mca_exe import source_amplitude

    class Handle:
        def source_power(self):
            return 2.7e7, 0.0
    th = types.SimpleNamespace(src_mtype=3, src_flx=1.7, src_the=150.0, dx=250.0, nx=5, dy=330.0, ny=3)
    assert source_amplitude(Handle(), th) == ref.amplitude('thermal', src_flx=1.7, ptot=2.7e7, lx=1250.0, ly=990.0)
    so = types.SimpleNamespace(src_mtype=1, src_flx=1.7, src_the=150.0, dx=250.0, nx=5, dy=330.0, ny=3)
    assert abs(source_amplitude(None, so)-ref.solar_amplitude(1.7, 150.0)) <= 2.0*np.spacing(1.5)
