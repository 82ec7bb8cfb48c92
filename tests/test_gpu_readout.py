"""
The last multiplication before the user: every route from raw float64 tallies to the float32 numbers of a result, held to a plain
float64 restatement of include/mi3d.h (tests/readout_ref.py) on tallies that are WRITTEN, not simulated.

The routes: mi3d_get_radiance / _flux / _heating (k_get_field, k_get_net_heating), mi3d_stats_add / _end_run / _get (k_stats_add,
k_stats_fold, k_stats_final), JobRunner._normalise (torch, the batched file route of several ranks) and the analytic parts
mi3d_get_direct_levels / mi3d_get_camera_direct.  Set-up of every test: caller-owned float64 torch buffers are bound, the scene is loaded
and ONE photon is run so that the handle has its source and its direct levels, mi3d_sync; nothing is folded into bound buffers after
that (k_fold_rad and the record sums of a flux run are queued by mi3d_run or joined by mi3d_sync; the lazy join of "overlap_sort" 2 is
for the handle's own buffers only).  Then the buffers are overwritten with patterns -- zeros, ones, magnitudes log-uniform over
1e-30 ... 1e10, and rounding probes: tallies t = m / norm with m the float64 midpoint of a float32 value and its successor, which any
float32 intermediate, fused multiply-add or reordered product rounds the other way -- and read out through every entry point.

Scenes: 5 x 3 columns, nine layers of unequal thickness (some not float32 numbers), 3-D layers 3-6, so that the analytic direct levels
are non-zero above the region and zero inside it; 12 x 10 x 28 for element counts (450; 10 440) that are no multiples of 256 and span
many blocks; three satellite views; cameras of 7 x 5 pixels, polar and rectangular map; sun, thermal emission, both.

Bounds
  k_get_field (radiance, flux, solar heating)   bit-equal: float64, unfused, rounded once, and the amplitude is the library's own double
                (the top level of mi3d_get_direct_levels, where tau = 0; mi3d_get_source_power) -- numpy repeats it exactly.  The solar
                amplitude itself is held to Src_flx |cos| from numpy to 2 double ulps.
  k_get_net_heating   E = mi3d_get_emission (float32), A the reference's absorbed part: |net - (A - E)| <= 2^-24 (|net| + |E|) 1.01
                + 2^-24 |A|.  The last term: the thermal path divides by the float32 LayerRec::dz where the solar path divides by the
                float64 grid difference; rounding dz to nearest moves 1 / dz by at most 2^-24 of itself.
  k_stats_add   the run field bit-equal to float32(t norm + a) * f summed in float32, job by job.
  k_stats_final the mean is (float)(sum * (1 / nrun)): a product with the reciprocal, not a division.  Two runs: 1 / 2 is exact and the
                mean bit-equal to float32(sum / 2).  Three runs: the reciprocal is rounded, so <= 1 ulp32 is what is owed and asserted.
                |sdev - ref| <= 2^-24 ref + 2^-25 |mean|: one float32 rounding, and the float64 cancellation of sum(x^2) / n - m^2
                (about 4 x 2^-53 m^2 before the root).
  JobRunner._normalise   bit-equal to Mi3dSolver.radiance / flux / heating of the same handle, for the sources and targets run_batched
                serves: the sun with every target, thermal flux and thermal satellite radiance.

Observed on an MI355X (printed by every test; a ratio above 1 fails):
  elements not bit-equal: k_get_field radiance 0, flux 0, heating 0; k_stats_add 0; mean of two runs 0; _normalise 0
  mean of three runs: 0 ulp32 off float32(sum / 3) in every element of the sixteen cases (1 is what is owed)
  largest ratio to the bound: net heating 0.854 (thermal), 0.975 (solar+thermal), both on the probes of the 28-layer scene, which sit
  where the one float32 rounding is worth nearly 2^-24 of the value: the bound is not slack; deviation 0.704
  a field whose runs are identical (reference deviation 0): the device returns exactly 0 in every element

Found by this module: JobRunner._normalise scaled every job with Src_flx mu0.  A thermal flux or thermal satellite-radiance simulation
of several jobs under several ranks (files kept, no abs_obj) goes through run_batched, and rank 0 wrote files off by
P_tot / (Lx Ly mu0).  Observed with the parent commit's mca_exe.py: its _normalise on the written tallies of the 5 x 3 thermal scene
gave 1 / 51.676658 of mi3d_get_flux and of mi3d_get_radiance in every element (P_tot / (Lx Ly mu0) = 51.676658; 59.36 on the
12 x 10 x 28 scene), and test_two_ranks_batched_thermal_files_match_one_rank failed with the two ranks' files at 0.038227 = 1 / 26.1597
(first g) and 0.005825 = 1 / 171.67 (second g) of one rank's in total-down, up and the radiance of all four jobs of either target (the
direct-down plane 0 in both), and the fused route up to 172 times the g-weighted mean of such files.  run_batched now records each
job's amplitude from its handle (mca_exe.source_amplitude); both tests pass.  The C read-outs needed no change.

Mutations (scratch builds, none committed) and the tests of this module each one fails:
  (float)t * (float)norm in k_get_field                      24 tests fail: radiance (7), flux (6), flux planes, solar heating (2),
                                                             _normalise (8)
  i > down_lo for i >= down_lo in k_get_field                11: flux (6), flux planes, _normalise with a flux tally (4)
  level index modulo nlevel - 1 in k_get_field               7: flux of the solar scenes (the direct levels; 2), flux planes, solar heating
                                                             (the thicknesses; 2), _normalise solar flux + heating (2)
  the analytic term added to plane 2 in k_get_field          5: flux of the solar scenes (2), flux planes, _normalise solar flux (2)
  v * f formed in float64 in k_stats_add                     UNDETECTABLE, all tests pass: the product of two float32 numbers has 48
                                                             significant bits and is exact in float64; rounding it to float32 once IS
                                                             the float32 product.  (A SUM kept in float64, acc + v f rounded once,
                                                             would differ, as a fused multiply-add does.)
  i > down_lo in k_stats_add                                 6: test_run_field_and_statistics[flux-*]
  level index modulo nlevel - 1 in k_stats_add               16: every case of test_run_field_and_statistics (factor and direct level)
  the old Src_flx mu0 for a thermal job in run_batched       4: test_normalise_is_the_c_read_out[thermal-*] (3) and the two-rank test
"""

import contextlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_HEAT, TARGET_RADIANCE
from tests import readout_ref as ref

pytestmark = pytest.mark.gpu

U32 = ref.U32
FH = TARGET_FLUX | TARGET_HEAT
N = 1000003                      # photons the tallies are said to hold: odd, so that no factor is a short binary fraction
NPROBE = 4096
SOURCES = ('solar', 'thermal', 'solar+thermal')


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------

def scene(source='solar', size='small', target=FH, sensor=None):
    """the scenes of the module docstring; sensor: None, 'satellite', 'polar', 'rect'"""
    rng = np.random.default_rng(11)
    if size == 'small':
        nx, ny, nz3, iz3l = 5, 3, 4, 3
        zgrd = np.array([0.0, 137.3, 300.0, 512.5, 700.1, 1000.0, 1450.0, 2100.7, 3500.0, 6000.0])
    else:
        nx, ny, nz3, iz3l = 12, 10, 6, 4
        zgrd = np.concatenate([[0.0], np.cumsum(90.0+37.7*rng.uniform(0.5, 4.0, 28))])
    nz = zgrd.size-1
    zm = 0.5*(zgrd[:-1]+zgrd[1:])
    kw = dict(zgrd=zgrd, ext1d=1.2e-5*np.exp(-zm/8000.0), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=np.full(nz, 2.0e-5),
              nx=nx, ny=ny, dx=250.0, dy=330.0, nz3=nz3, iz3l=iz3l, extp=rng.uniform(1.0e-3, 2.0e-2, (1, nz3, ny, nx)),
              omgp=np.full((1, nz3, ny, nx), 0.97), apfp=np.full((1, nz3, ny, nx), 0.85), sfc_mtype=1, sfc_param=[0.1, 0, 0, 0, 0],
              src_flx=1.7, src_the=150.0, src_phi=270.0, target=target)
    if source != 'solar':
        kw.update(src_mtype=3 if source == 'thermal' else 2, src_wlen=10.8 if source == 'thermal' else 3.9,
                  tmp1d=np.linspace(290.0, 215.0, nz+1), tmpa3d=rng.uniform(-3.0, 3.0, (nz3, ny, nx)))
        if source == 'solar+thermal':
            kw.update(src_fsol=12.5)
    if sensor == 'satellite':
        kw.update(view_the=[180.0, 153.9, 134.4], view_phi=[0.0, 0.0, 180.0], view_zloc=[705000.0]*3, nxr=7, nyr=5)
    elif sensor in ('polar', 'rect'):
        kw.update(rad_kind=1, view_the=[0.0, 180.0, 40.0], view_phi=[0.0, 0.0, 30.0], view_zloc=[0.0, 3000.0, 100.0], nxr=7, nyr=5,
                  cam_xpos=[0.5, 0.3, 0.7], cam_ypos=[0.5, 0.6, 0.2], cam_apsize=[0.05]*3, cam_images=0)
        if sensor == 'rect':
            kw.update(cam_mpmap=2, cam_umax=[90.0]*3, cam_vmax=[180.0]*3)
        else:
            kw.update(cam_qmax=[178.0]*3)
    return Scene(**kw)


class Loaded:
    """a handle with the scene loaded, one photon run and its tallies in caller-owned float64 buffers: slices of ONE row, as
    JobRunner.run_batched lays them out"""

    def __init__(self, solver, sc):
        import torch
        self.torch, self.sol, self.sc = torch, solver, sc
        self.dev = torch.device('cuda', solver.device)
        self.sizes = (max(sc.nview, 1)*sc.nyr*sc.nxr if sc.target & TARGET_RADIANCE else 0,
                      3*(sc.nz+1)*sc.ny*sc.nx if sc.target & TARGET_FLUX else 0,
                      sc.nz*sc.ny*sc.nx if sc.target & TARGET_HEAT else 0)
        a, b, c = self.sizes
        self.row = torch.zeros(a+b+c, dtype=torch.float64, device=self.dev)
        self.rad, self.flux, self.heat = self.row[:a], self.row[a:a+b], self.row[a+b:]
        ptr = lambda t: t.data_ptr() if t.numel() else None
        solver.load_scene(sc)
        solver.set_counting(False)
        solver.bind(rad_ptr=ptr(self.rad), flux_ptr=ptr(self.flux), stream=torch.cuda.current_stream(self.dev).cuda_stream, heat_ptr=ptr(self.heat))
        solver.reset()
        solver.run(1, seed=3)
        solver.sync()
        torch.cuda.synchronize(self.dev)
        self.lx, self.ly = sc.dx*sc.nx, sc.dy*sc.ny
        self.direct = solver.direct_levels()
        self.kind = {1: 'solar', 2: 'solar+thermal', 3: 'thermal'}[sc.src_mtype]
        if self.kind == 'solar':
            self.amp = ref.amplitude('solar', direct_top=self.direct[-1])
        else:
            ptot, psol = solver.source_power()
            self.amp = ref.amplitude(self.kind, src_flx=sc.src_flx, ptot=ptot, psol=psol, lx=self.lx, ly=self.ly)
        self.dz = np.diff(sc.zgrd)

    def write(self, rad=None, flux=None, heat=None):
        for buf, arr in ((self.rad, rad), (self.flux, flux), (self.heat, heat)):
            if arr is not None:
                buf.copy_(self.torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64).ravel()))
        self.torch.cuda.synchronize(self.dev)

    def rad_norm(self, n=N):
        sc = self.sc
        return ref.radiance_norm(self.amp, 'camera' if sc.rad_kind == 1 else 'satellite', n, sc.nxr, sc.nyr, self.lx, self.ly)

    def field_norm(self, n=N):
        return ref.field_norm(self.amp, n, self.sc.nx, self.sc.ny)


@contextlib.contextmanager
def loaded(solver, sc):
    try:
        yield Loaded(solver, sc)
    finally:
        solver.bind(None, None, None)
        solver.stats_set_analytic_share(1.0)


def patterns(shape, seed, probe):
    """the written tallies: (name, array).  probe(m) -> the tallies that put float64 midpoints m (an array of `shape`) at the rounding"""
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    yield 'zeros', np.zeros(shape)
    yield 'ones', np.ones(shape)
    yield 'log-uniform', 10.0**rng.uniform(-30.0, 10.0, shape)
    for q in range(-(-NPROBE//size)):
        yield 'probes %d' % q, probe(seed*100+q)


def count_unequal(name, got, want, tag):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    bad = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
    print('%-28s %-12s elements not bit-equal: %d of %d' % (tag, name, bad, got.size), '' if not bad else '(largest distance %d ulp32)' % ref.ulps32(got, want).max())
    return bad


# ---- the amplitude and the analytic direct levels ----------------------------------------------------------------------------------------

def test_amplitude_and_direct_levels(solver):
    with loaded(solver, scene('solar')) as L:
        sc = L.sc
        want = ref.solar_amplitude(sc.src_flx, sc.src_the)
        print('solar amplitude: library %.17g, numpy %.17g' % (L.amp, want))
        assert abs(L.amp-want) <= 2.0*np.spacing(want)
        k_top = sc.iz3l-1+sc.nz3                          # the first level above the 3-D region
        assert np.all(L.direct[:k_top] == 0.0) and np.all(L.direct[k_top:] > 0.0) and np.all(np.diff(L.direct[k_top:]) > 0.0)
        # Src_flx mu0 exp(-tau / mu0) from the 1-D layers above the region
        b = (sc.abs1d.astype(np.float64)+sc.ext1d.astype(np.float64).sum(axis=0))*L.dz
        tau = np.concatenate([np.cumsum(b[::-1])[::-1], [0.0]])[k_top:]
        mu0 = L.amp/sc.src_flx
        assert np.allclose(L.direct[k_top:], L.amp*np.exp(-tau/mu0), rtol=1.0e-13, atol=0.0)
    for source in ('thermal', 'solar+thermal'):
        with loaded(solver, scene(source)) as L:
            assert L.direct.shape == (L.sc.nz+1,) and np.all(L.direct == 0.0)          # no analytic direct beam: the levels are off
            ptot, psol = solver.source_power()
            assert ptot > 0.0 and (psol > 0.0) == (source == 'solar+thermal')
            if source == 'solar+thermal':
                want = L.sc.src_fsol*abs(np.cos(np.deg2rad(L.sc.src_the)))*L.lx*L.ly
                assert abs(psol-want) <= 4.0*np.spacing(want)


# ---- k_get_field -------------------------------------------------------------------------------------------------------------------------

RAD_CASES = [(so, se) for so in SOURCES for se in ('satellite', 'polar', 'rect') if not (so == 'solar+thermal' and se != 'satellite')]
# (cameras of a solar+thermal job: MI3D_EUNSUP from mi3d_run, asserted by tests/test_gpu_source_mix.py)


@pytest.mark.parametrize('source,sensor', RAD_CASES, ids=['%s-%s' % c for c in RAD_CASES])
def test_radiance_is_the_header_formula(solver, source, sensor):
    with loaded(solver, scene(source, sensor=sensor, target=TARGET_RADIANCE)) as L:
        sc = L.sc
        shape = (sc.nview, sc.nyr, sc.nxr)
        norm = L.rad_norm()
        bad = 0
        for name, t in patterns(shape, 21, lambda s: ref.probes(shape, s)[0]/norm):
            L.write(rad=t)
            got = solver.radiance(N)
            want = ref.radiance(t, L.amp, 'camera' if sc.rad_kind == 1 else 'satellite', N, sc.nxr, sc.nyr, L.lx, L.ly)
            bad += count_unequal(name, got, want, 'radiance %s %s' % (source, sensor))
        assert bad == 0
        if sc.rad_kind == 1:
            cd = solver.camera_direct()
            assert cd.shape == shape
            if source == 'thermal':
                assert np.all(cd == 0.0)                       # no sun
            else:
                # the up-looking camera sees the sun (30 degrees off its axis) in one pixel, the down-looking one does not
                assert np.count_nonzero(cd[0]) == 1 and np.all(cd[1] == 0.0) and np.all(cd >= 0.0)


@pytest.mark.parametrize('size', ['small', 'large'])
@pytest.mark.parametrize('source', SOURCES)
def test_flux_is_the_header_formula(solver, source, size):
    with loaded(solver, scene(source, size)) as L:
        sc = L.sc
        shape = (3, sc.nz+1, sc.ny, sc.nx)
        assert int(np.prod(shape)) == (450 if size == 'small' else 10440)
        norm = L.field_norm()
        a = L.direct[None, :, None, None]

        def probe(s):
            # plane 0: t0 norm + a = m0; plane 1: (t0 + t1) norm + a = m1 > m0; plane 2: t2 norm = m2
            m0 = ref.probes(shape[1:], s, 0.5, 8.0)[0]
            m1 = ref.probes(shape[1:], s+50, 8.5, 12.0)[0]
            m2 = ref.probes(shape[1:], s+70, -20.0, 8.0)[0]
            t0 = (m0-a[0])/norm
            return np.stack([t0, (m1-a[0])/norm-t0, m2/norm])
        bad = 0
        for name, t in patterns(shape, 31, probe):
            assert np.all(t >= 0.0)
            L.write(flux=t)
            bad += count_unequal(name, solver.flux(N), ref.flux(t, L.amp, L.direct, N), 'flux %s %s' % (source, size))
        assert bad == 0


def test_flux_planes_direct_total_up_and_the_analytic_term_on_the_first_two_only(solver):
    """three recognisable planes: direct-down a few units, diffuse-down thousands, up millions"""
    with loaded(solver, scene('solar')) as L:
        sc = L.sc
        nl, ncol = sc.nz+1, sc.ny*sc.nx
        idx = np.arange(nl*ncol, dtype=np.float64).reshape(nl, sc.ny, sc.nx)
        raw = np.stack([1.0+idx/1024.0, 4096.0+idx, 4194304.0+3.0*idx])
        L.write(flux=raw)
        f = solver.flux(N)
        norm = L.field_norm()
        d = L.direct[:, None, None]
        assert np.count_nonzero(d) == 4                            # (so that a term on the wrong plane or level shows)
        assert np.array_equal(f[0], (raw[0]*norm+d).astype(np.float32))
        assert np.array_equal(f[1], ((raw[0]+raw[1])*norm+d).astype(np.float32))            # elements [down_lo, 2 down_lo): direct + diffuse
        assert np.array_equal(f[2], (raw[2]*norm).astype(np.float32))                      # untouched by either
        # the first element of the total-down plane, i == down_lo, holds its direct part as every other one
        assert f[1, 0, 0, 0] == np.float32((raw[0, 0, 0, 0]+raw[1, 0, 0, 0])*norm+d[0, 0, 0])
        assert f[1, 0, 0, 0] != np.float32(raw[1, 0, 0, 0]*norm+d[0, 0, 0])


@pytest.mark.parametrize('size', ['small', 'large'])
def test_solar_heating_is_the_header_formula(solver, size):
    with loaded(solver, scene('solar', size)) as L:
        sc = L.sc
        shape = (sc.nz, sc.ny, sc.nx)
        norm = L.field_norm()
        assert np.any(L.dz.astype(np.float32).astype(np.float64) != L.dz)      # thicknesses that a float32 divisor would change
        bad = 0
        for name, t in patterns(shape, 41, lambda s: ref.probes(shape, s)[0]*L.dz[:, None, None]/norm):
            L.write(heat=t)
            bad += count_unequal(name, solver.heating(N), ref.heating(t, L.amp, L.dz, N), 'heating solar %s' % size)
        assert bad == 0


# ---- k_get_net_heating -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('source', ['thermal', 'solar+thermal'])
def test_net_heating_is_absorbed_minus_emitted(solver, source):
    worst = 0.0
    for size in ('small', 'large'):
        with loaded(solver, scene(source, size)) as L:
            sc = L.sc
            shape = (sc.nz, sc.ny, sc.nx)
            E = solver.emission()
            assert E.shape == shape and np.all(E > 0.0)
            norm = L.field_norm()
            balance = E.astype(np.float64)*L.dz[:, None, None]/norm         # absorbed = emitted: the net is what rounding leaves
            rng = np.random.default_rng(5)
            cases = list(patterns(shape, 51, lambda s: ref.probes(shape, s)[0]*L.dz[:, None, None]/norm))
            cases += [('balance', balance), ('near balance', balance*(1.0+rng.uniform(-1.0e-6, 1.0e-6, shape)))]
            for name, t in cases:
                L.write(heat=t)
                net = solver.heating(N).astype(np.float64)
                A, want = ref.net_heating(t, L.amp, L.dz, E, N)
                bound = U32*(np.abs(net)+np.abs(E))*1.01+U32*np.abs(A)
                ratio = float((np.abs(net-want)/bound).max())
                print('net heating %s %s %-12s largest |net - (A - E)| / bound: %.3f' % (source, size, name, ratio))
                worst = max(worst, ratio)
                assert np.all(np.isfinite(net)) and ratio <= 1.0
                if name == 'zeros':
                    assert np.array_equal(net, -E.astype(np.float64))       # pure cooling: 0 - e rounds to -E
    print('net heating %s: largest ratio to the bound %.3f' % (source, worst))


# ---- k_stats_add, k_stats_fold, k_stats_final ------------------------------------------------------------------------------------------------

STATS_CASES = [('flux', 'solar', None), ('flux', 'thermal', None), ('flux', 'solar+thermal', None), ('rad', 'solar', 'satellite'),
               ('rad', 'thermal', 'satellite'), ('rad', 'solar', 'polar'), ('rad', 'solar', 'rect'), ('rad', 'thermal', 'rect')]


@pytest.mark.parametrize('share', [1.0, 0.0])
@pytest.mark.parametrize('what,source,sensor', STATS_CASES, ids=['-'.join(str(x) for x in c if x) for c in STATS_CASES])
def test_run_field_and_statistics(solver, what, source, sensor, share):
    """3 jobs x 2 runs (and a third run for the rounded reciprocal), per-level / per-view factors that are not 1, other photon numbers
    from job to job; then a session whose two runs are identical"""
    which = TARGET_FLUX if what == 'flux' else TARGET_RADIANCE
    with loaded(solver, scene(source, 'small', target=which, sensor=sensor)) as L:
        sc = L.sc
        rng = np.random.default_rng(61)
        if what == 'flux':
            shape = (3, sc.nz+1, sc.ny, sc.nx)
            fshape = (1, sc.nz+1, 1, 1)
        else:
            shape = (sc.nview, sc.nyr, sc.nxr)
            fshape = (sc.nview, 1, 1)
        add_px = None
        if what == 'rad' and sensor == 'rect' and source == 'solar':
            add_px = solver.camera_direct()                     # the direct sun joins the run field of rectangular-map cameras
            assert np.count_nonzero(add_px) >= 1

        def job(t, n, f):
            if what == 'flux':
                tt, a = ref.flux_terms(t, L.direct, share)
                return tt, L.field_norm(n), a, f.reshape(fshape)
            return t, L.rad_norm(n), (add_px*share if add_px is not None else 0.0), f.reshape(fshape)

        def one_run(tallies, key):
            jobs = []
            for j, t in enumerate(tallies):
                n = N+1000*j
                f = (0.2+rng.uniform(0.0, 1.0, fshape[0] if what == 'rad' else fshape[1])).astype(np.float32)
                L.write(**{what if what == 'rad' else 'flux': t})
                solver.stats_add(n, factor_rad=f if what == 'rad' else None, factor_flux=f if what == 'flux' else None)
                jobs.append(job(t, n, f))
            got = solver.stats_end_run(keep=True)[key]
            want = ref.run_field(jobs)
            return got, want

        key = 'flux' if what == 'flux' else 'rad'
        solver.stats_begin()
        solver.stats_set_analytic_share(share)
        bad, fields = 0, []
        for r in range(3):
            tallies = [10.0**rng.uniform(-6.0, 6.0, shape) for _ in range(3)]
            if r == 0:
                tallies[1] = ref.probes(shape, 77)[0]/(L.field_norm(N+1000) if what == 'flux' else L.rad_norm(N+1000))
            got, want = one_run(tallies, key)
            bad += count_unequal('run %d' % r, got, want, 'run field %s %s %s' % (what, source, sensor))
            fields.append(got)
            if r == 0:
                continue
            mean, sdev, nrun = solver.stats_get(which)
            assert nrun == r+1
            m64, s64 = ref.run_stats(fields)
            if nrun == 2:
                bad += count_unequal('mean of 2', mean, m64.astype(np.float32), 'statistics')
            else:
                d = int(ref.ulps32(mean, m64.astype(np.float32)).max())
                print('statistics: mean of 3 runs, largest distance to float32(sum / 3): %d ulp32' % d)
                assert d <= 1
            bound = U32*s64+0.5*U32*np.abs(m64)
            ok = bound > 0.0
            ratio = float((np.abs(sdev.astype(np.float64)-s64)[ok]/bound[ok]).max())
            print('statistics %s %s %s, %d runs: largest |sdev - ref| / bound %.3f' % (what, source, sensor, nrun, ratio))
            assert ratio <= 1.0 and np.all(sdev[~ok] == 0.0)
        assert bad == 0
        # two identical runs: the reference deviation is 0
        solver.stats_begin()
        solver.stats_set_analytic_share(share)
        tallies = [10.0**rng.uniform(-6.0, 6.0, shape) for _ in range(3)]
        state = rng.bit_generator.state
        g1, _ = one_run(tallies, key)
        rng.bit_generator.state = state                             # (the same factors again)
        g2, _ = one_run(tallies, key)
        assert np.array_equal(g1, g2)
        mean, sdev, nrun = solver.stats_get(which)
        assert nrun == 2 and np.array_equal(mean, g1)
        print('identical runs: largest deviation the device returns %.3e (largest / mean %.3e)' % (sdev.max(), (sdev/np.maximum(mean, 1e-30)).max()))
        assert np.all(sdev.astype(np.float64) <= 0.5*U32*np.abs(mean.astype(np.float64)))


# ---- JobRunner._normalise ----------------------------------------------------------------------------------------------------------------

NORMALISE_CASES = [('solar', FH, None, 'small'), ('solar', FH, None, 'large'), ('solar', TARGET_RADIANCE, 'satellite', 'small'),
                   ('solar', TARGET_RADIANCE, 'polar', 'small'), ('solar', TARGET_RADIANCE, 'rect', 'small'), ('thermal', TARGET_FLUX, None, 'small'),
                   ('thermal', TARGET_FLUX, None, 'large'), ('thermal', TARGET_RADIANCE, 'satellite', 'small')]


@pytest.mark.parametrize('source,target,sensor,size', NORMALISE_CASES, ids=['%s-%s-%s' % (c[0], c[2] or {FH: 'flux+heat', TARGET_FLUX: 'flux'}[c[1]], c[3])
                                                                             for c in NORMALISE_CASES])
def test_normalise_is_the_c_read_out(solver, source, target, sensor, size):
    """what rank 0 of the batched file route makes of a row of all-reduced tallies against mi3d_get_* of the same handle on the same
    buffers, for every source x target run_batched serves"""
    from er3t_amd.rtm.mca.mca_exe import JobRunner, source_amplitude, wants_rdir
    with loaded(solver, scene(source, size, target=target, sensor=sensor)) as L:
        sc = L.sc
        amp = source_amplitude(solver, sc)
        print('amplitude: run_batched %.17g, the library %.17g; P_tot / (Lx Ly mu0) = %.4f' % (amp, L.amp, L.amp/(sc.src_flx*sc.mu0)))
        assert amp == L.amp
        if source == 'thermal':
            assert abs(L.amp/(sc.src_flx*sc.mu0)-1.0) > 0.01          # (the solar factor cannot pass by accident)
        meta = dict(scene=sc, nphoton=N, direct=L.direct if target & TARGET_FLUX else None, rdir=solver.camera_direct() if wants_rdir(sc) else None,
                    norm=dict(amp=amp, rad_kind=sc.rad_kind, lx=sc.dx*sc.nx, ly=sc.dy*sc.ny, dz=np.diff(sc.zgrd)))
        a, b, c = L.sizes
        rng = np.random.default_rng(71)
        bad = 0
        for q in range(4):
            t = [np.zeros(a+b+c), np.ones(a+b+c), 10.0**rng.uniform(-30.0, 10.0, a+b+c), None][q]
            if t is None:                                            # probes, each part on its own factor
                m = ref.probes((a+b+c,), 5, 0.5, 8.0)[0]
                t = m/(L.rad_norm() if a else L.field_norm())
                if c:
                    t[a+b:] = (m[a+b:].reshape(sc.nz, -1)*L.dz[:, None]).ravel()/L.field_norm()
            L.write(rad=t[:a] if a else None, flux=t[a:a+b] if b else None, heat=t[a+b:] if c else None)
            out = {k: v.cpu().numpy() for k, v in JobRunner._normalise(L.row, L.sizes, meta).items()}
            if a:
                bad += count_unequal('rad %d' % q, out['rad'], solver.radiance(N), '_normalise %s' % source)
                assert ('rdir' in out) == wants_rdir(sc)
                if 'rdir' in out:
                    assert np.array_equal(out['rdir'], solver.camera_direct().astype(np.float32))
            if b:
                bad += count_unequal('flux %d' % q, out['flux'], solver.flux(N), '_normalise %s' % source)
            if c:
                bad += count_unequal('heat %d' % q, out['heat'], solver.heating(N), '_normalise %s' % source)
        assert bad == 0


def test_the_batched_route_still_refuses_what_it_cannot_normalise(solver, monkeypatch):
    """solar+thermal jobs, the net heating rate of a thermal job, thermal cameras: refused before anything runs or is exchanged"""
    from er3t_amd.rtm.mca import mca_exe
    runner = mca_exe.JobRunner(device=0)
    refused = [(scene('solar+thermal', target=TARGET_FLUX), 'solar\\+thermal job'), (scene('thermal', target=FH), 'net heating rate of a thermal job'),
               (scene('thermal', target=TARGET_RADIANCE, sensor='polar'), 'cameras and point radiometers of a thermal job'),
               (scene('thermal', target=TARGET_RADIANCE, sensor='rect'), 'cameras and point radiometers of a thermal job')]
    monkeypatch.setattr(mca_exe, 'mca_inp_read', lambda fname: {})
    try:
        for sc, text in refused:
            monkeypatch.setattr(runner, 'load', lambda nml, fdir, solver, slot=0, sc=sc: sc)
            with pytest.raises(OSError, match='%s.*not served by the batched route' % text):
                runner.run_batched([('a.inp.txt', 'a.out.bin', 1000), ('b.inp.txt', 'b.out.bin', 1000)], 0)
    finally:
        for sol in runner.sols:
            sol.close()


# ---- two ranks: the batched file route of thermal flux and thermal satellite radiance ----------------------------------------------------

def test_two_ranks_batched_thermal_files_match_one_rank(tmp_path):
    """two ranks under torch.distributed.run ('gloo', both on this box's one GPU; tests/readout_dist_worker.py): thermal flux and thermal
    satellite radiance, two g x two runs with the files kept and no abs_obj, so that mca_run takes JobRunner.run_batched; rank 0 then runs
    every input file again alone.  Every variable of every job file agrees to rtol 2e-7 -- equal histories whose float64 sums fall in
    another order, rounded to float32 once; the direct-down plane is 0 in both.  The fused route over the same job files agrees with the
    g-weighted mean of the files to rtol 1e-6: both are sums of a few positive float32 terms, at most 16 float32 roundings between them
    (per job a normalisation, a product and a sum on either route, on the fused route per rank, then the exchange's sum and the mean)."""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'tests', 'readout_dist_worker.py'), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(os.path.join(out, 'result.npz'))
    wrong = []                                                        # (every variable is looked at before the test fails)
    for target, nvar in (('flux', 3), ('radiance', 1)):
        njob = int(z[target+'_njob'])
        assert njob == 4 and int(z[target+'_batched']) == 1
        for j in range(njob):
            factor = float(z['%s_factor_%d' % (target, j)])
            assert abs(factor-1.0) > 0.01, factor                     # P_tot / (Lx Ly mu0): the old amplitude cannot pass by accident
            for v in range(nvar):
                a, b = z['%s_dist_%d_%d' % (target, j, v)], z['%s_solo_%d_%d' % (target, j, v)]
                assert a.shape == b.shape and np.all(np.isfinite(a))
                ratio = float(np.median(a[b > 0.0]/b[b > 0.0])) if np.any(b > 0.0) else 1.0
                print('%s job %d variable %d: files of two ranks / one rank, median %.6f (P_tot / (Lx Ly mu0) = %.4f)' % (target, j, v, ratio, factor))
                if target == 'flux' and v == 0:
                    assert np.all(a == 0.0) and np.all(b == 0.0)      # a thermal job has no direct beam
                else:
                    assert b.max() > 0.0
                if not np.allclose(a, b, rtol=2.0e-7, atol=0.0):
                    wrong.append((target, 'job %d' % j, 'variable %d' % v, 'two ranks / one rank %.6f' % ratio))
        for k in ('f_up', 'f_down') if target == 'flux' else ('rad',):
            a, b = z['%s_fused_%s' % (target, k)], z['%s_files_%s' % (target, k)]
            assert a.shape == b.shape and b.max() > 0.0
            dev = float(np.abs(a/np.where(b > 0, b, 1.0)-1.0)[b > 0].max())
            print('%s %s: fused route / g-weighted mean of the files - 1, largest %.3e' % (target, k, dev))
            if not np.allclose(a, b, rtol=1.0e-6, atol=0.0):
                wrong.append((target, k, 'fused route against the files', dev))
    assert not wrong, wrong
