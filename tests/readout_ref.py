"""
The step from raw float64 tallies to the float32 numbers a user reads, restated in plain numpy float64 from the TEXT of include/mi3d.h
(mi3d_get_radiance, mi3d_get_flux, mi3d_get_direct_levels, mi3d_get_heating, mi3d_get_emission, mi3d_stats_*, mi3d_set_thermal,
mi3d_set_solar_irradiance) -- not from the kernels.  Reference of tests/test_gpu_readout.py and tests/test_readout_host.py.

What the header states, and what is restated here:

  amplitude   the power per unit domain area a job's photons stand for in all: Src_flx mu0 (solar), Src_flx P_tot / (Lx Ly) (thermal),
              Src_flx (P_tot + P_sol) / (Lx Ly) (solar+thermal)
  radiance    tally x amplitude x nxr nyr / N (satellite views), tally x amplitude x Lx Ly / N (cameras)
  flux        planes direct-down, total-down = direct + diffuse, up: tally x amplitude x nx ny / N, plus the known part of the direct beam
              (mi3d_get_direct_levels) on the first two planes only
  heating     tally x amplitude x nx ny / N / layer thickness; thermal and solar+thermal jobs: that, minus mi3d_get_emission
  run field   += factor[level] x normalised tally of the job, float32 product and float32 sum, job by job
  statistics  mean and population standard deviation over the closed runs

Every read-out is float64 in that order of operations and rounded to float32 once.  Lx = dx nx and Ly = dy ny are formed first.
"""

import numpy as np

U32 = 2.0**-24        # unit round-off of float32: |fl(x) - x| <= U32 |x|


def solar_amplitude(src_flx, src_the_deg):
    """Src_flx mu0, mu0 = |cos Src_the|, from numpy: what the library's own value is held to (2 double ulps) -- not what the other
    functions are given, so that a libm `cos` an ulp away cannot look like a kernel error"""
    return float(src_flx)*abs(np.cos(np.float64(src_the_deg)*np.pi/180.0))


def amplitude(kind, src_flx=1.0, direct_top=None, ptot=None, psol=0.0, lx=None, ly=None):
    """the amplitude of a job as the library's own double:
    'solar'          direct_top: the top level of mi3d_get_direct_levels in a scene whose top layer is 1-D, where tau = 0 and the level holds
                     Src_flx mu0 exp(-0) itself
    'thermal'        Src_flx P_tot / (Lx Ly), P_tot from mi3d_get_source_power
    'solar+thermal'  Src_flx (P_tot + P_sol) / (Lx Ly)"""
    if kind == 'solar':
        return float(direct_top)
    area = np.float64(lx)*np.float64(ly)
    if kind == 'thermal':
        return float(np.float64(src_flx)*np.float64(ptot)/area)
    if kind == 'solar+thermal':
        return float(np.float64(src_flx)*(np.float64(ptot)+np.float64(psol))/area)
    raise ValueError(kind)


def radiance_norm(amp, kind, nphoton, nxr=1, nyr=1, lx=None, ly=None):
    """what one unit of a radiance tally is worth: kind 'satellite' (Rad_mrkind = 2) or 'camera' (Rad_mrkind = 1)"""
    amp = np.float64(amp)
    if kind == 'camera':
        return amp*np.float64(lx)*np.float64(ly)/np.float64(nphoton)
    if kind == 'satellite':
        return amp*np.float64(nxr)*np.float64(nyr)/np.float64(nphoton)
    raise ValueError(kind)


def field_norm(amp, nphoton, nx, ny):
    """what one unit of a flux or heating tally is worth: amplitude x nx ny / N"""
    return np.float64(amp)*np.float64(nx)*np.float64(ny)/np.float64(nphoton)


def radiance(raw, amp, kind, nphoton, nxr=1, nyr=1, lx=None, ly=None):
    """(...,) float64 tallies -> float32 radiances"""
    return (np.asarray(raw, dtype=np.float64)*radiance_norm(amp, kind, nphoton, nxr, nyr, lx, ly)).astype(np.float32)


def flux_terms(raw, direct_levels=None, share=1.0):
    """(3, nz+1, ny, nx) raw planes direct-down, DIFFUSE-down, up -> (tally of every result plane, analytic term of every result plane) in
    float64: total-down = direct + diffuse; the known direct beam, times the analytic share, on planes 0 and 1 only"""
    raw = np.asarray(raw, dtype=np.float64)
    t = raw.copy()
    t[1] = raw[1]+raw[0]
    a = np.zeros_like(raw)
    if direct_levels is not None:
        a[:2] = (np.asarray(direct_levels, dtype=np.float64)*np.float64(share))[None, :, None, None]
    return t, a


def flux(raw, amp, direct_levels, nphoton):
    """(3, nz+1, ny, nx) raw planes -> float32 direct-down, total-down, up"""
    t, a = flux_terms(raw, direct_levels)
    return (t*field_norm(amp, nphoton, raw.shape[3], raw.shape[2])+a).astype(np.float32)


def heating64(raw, amp, dz, nphoton):
    """(nz, ny, nx) weights absorbed -> absorbed power per unit volume, float64 (the absorbed part A of a thermal job's net)"""
    raw = np.asarray(raw, dtype=np.float64)
    return raw*field_norm(amp, nphoton, raw.shape[2], raw.shape[1])/np.asarray(dz, dtype=np.float64)[:, None, None]


def heating(raw, amp, dz, nphoton):
    """a solar job's heating rates, float32"""
    return heating64(raw, amp, dz, nphoton).astype(np.float32)


def net_heating(raw, amp, dz, emission, nphoton):
    """a thermal or solar+thermal job: (A, A - E) in float64, A the absorbed part, E mi3d_get_emission (float32, the term the library takes
    off).  Not rounded: the library works E out on the device, so the test holds it to a bound, not to these bits"""
    A = heating64(raw, amp, dz, nphoton)
    return A, A-np.asarray(emission, dtype=np.float32).astype(np.float64)


def run_field(jobs):
    """the per-run field of mi3d_stats_add: jobs = [(tally float64, norm, analytic term float64 or 0.0, factor float32 broadcastable)] in
    job order; per job v = float32(tally x norm + term), then a float32 product with the factor and a float32 sum"""
    acc = None
    for t, norm, a, f in jobs:
        v = (np.asarray(t, dtype=np.float64)*np.float64(norm)+np.asarray(a, dtype=np.float64)).astype(np.float32)
        prod = v*np.asarray(f, dtype=np.float32)
        acc = (np.zeros_like(prod) if acc is None else acc)+prod          # (the field starts at +0)
        assert prod.dtype == np.float32 and acc.dtype == np.float32
    return acc


def run_stats(fields):
    """mean and population standard deviation over the runs' float32 fields, two-pass in float64: (mean64, sdev64)"""
    x = np.stack([np.asarray(f, dtype=np.float32) for f in fields]).astype(np.float64)
    n = x.shape[0]
    mean = x.sum(axis=0)/n
    return mean, np.sqrt(((x-mean[None])**2).sum(axis=0)/n)


def ulps32(a, b):
    """distance of two float32 arrays in units in the last place (finite values of one sign or zero)"""
    ia = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia-ib)


def probes(n, seed, lo=-20.0, hi=8.0):
    """n float64 midpoints m between a float32 value f (magnitudes 10^lo ... 10^hi) and its successor, with f: a float64 result that
    lands on either side of m rounds to f or to its successor -- any float32 intermediate, fused multiply-add or reordered product
    moves some of them across"""
    rng = np.random.default_rng(seed)
    f = (10.0**rng.uniform(lo, hi, n)).astype(np.float32)
    g = np.nextafter(f, np.float32(np.inf))
    return 0.5*(f.astype(np.float64)+g.astype(np.float64)), f
