"""
The flux loops' flights against float64, photon by photon (reference, scenes and launches: tests/flight_ref.py, held to
the CPU oracle by tests/test_flight_host.py).

Scenes in which nothing scatters, wmin = 0, a black or a Lambert surface (albedo 0.5): a collision leaves the photon's whole weight in ONE
heating cell, every level crossed is ONE tally of that weight in ONE column.  The raw float64 tallies, read through bound buffers, are sums
of 1 and 0.5 and are predicted element by element from the photons' Philox blocks.  Every launch asserts

  flux      lower <= raw <= upper, raw a multiple of 0.5 bit for bit, raw exactly 0 where no photon can come (upper = 0; the direct plane at
            the analytic levels >= kdir and the whole diffuse-down plane among them)
  heat      the same with the ONE allowance HEAT_REL = 2^-22 relative (see below); exactly 0 where no photon can collide
  totals    heat, photons into the surface, photons through the top inside their bounds
  read-out  solver.flux and solver.heating between the bounds normalised as tests/readout_ref.py normalises (float32 rounding is monotone),
            the analytic direct levels as the reference's own exp(-tau / mu0) to 1e-12
  route     kernel_name() is the route the launch is there for; every tuning is restored
  counting  (one launch per route) photons, surface, escaped, absorbed and flux_tally inside the predicted bounds; the same raw tallies

HEAT_REL.  A collision deposits w_in (bt - kstot) rcp(bt) (mi3d_kernel_flux.hip, blocks C and B2; k_transport likewise): with kstot = 0 that
is w_in times bt rcp(bt) in float32, v_rcp_f32 good to one ulp -- 1 within 2^-23 + 2^-24 < 2^-22, not 1.  A property of the formula, the
same for every photon whatever its path; the flux tallies carry the weight itself and stay exact.

The drop list (uncertain photons add to upper bounds only) and its margins: tests/flight_ref.py.  At most 3 % of a launch may be dropped
and at least 10000 of 20000 (2500 of 3000) photons are compared: asserted on the host, test_flight_host.py.

Path-length launches (Flx_mhest = 1): the flux planes as above; heat per cell within max(4 E_emul, 8 EPS) x sum|terms| of the certain
photons' float64 sum of w kappa_a l -- below with nothing else allowed (every term is positive, the uncertain photons can only add), above
plus the uncertain photons' share.  E_emul: the float32 emulation's largest error of a cell's sum relative to that sum over the class (scene,
sun, solver; 3000 photons), never a figure the GPU gave.  A flight through a horizontally uniform layer leaves ONE term in the column of the
piece's midpoint (the estimator's definition, include/mi3d.h); a midpoint within 2 m(t) of a column face makes that term uncertain.

Launches (flight_ref.LAUNCHES), each named for what it reaches:
  default-*      k_transport_flux<.,0,0|1> with lists and runs: every scene variant at the slant sun (150, 37), both surfaces; on base and
                 stacked also the vertical sun, along +x with u_y = +0 and -0, along -y, grazing (105, 200); the diagonal on diag
  no_runs, atomics, full_lists (tlcap_log2 = 17: the lists run full, the rest goes out as atomics), cap16 (tlcap_log2 = 16: too small for
                 lists, atomics), small (3000 photons: no sort, no lists), offset (ids beyond 2^33), tiles (tile_cols = 4)
  solver1-*, solver2-*   <.,1,.> partial 3-D, and the column-bound flights of independent columns
  mix2-*         two 1-D constituents (MIX 2); default-two-*: two 3-D constituents (MIX 1)
  general-*      set_kernel(general=True): k_transport<.,0,1,.>
  path-*         Flx_mhest = 1 builds

Measured on an MI355X (profiles/r25/new_tests.log; 101 tests in 10 s).  Every launch passed as first run: no kernel changed.
  route                                         launches   photons compared per launch   dropped         largest ratio to the bound
  default flux loop, lists and runs             44         19806 - 19986 of 20000        0.07 - 0.97 %   exact
  no_runs, atomics, full_lists, cap16, tiles    2 each     19877, 19879                  0.60, 0.61 %    exact
  small (3000 photons) / offset beyond 2^33     2 / 2      2983, 2986 / 19878, 19882     0.47 - 0.61 %   exact
  solver 1 (<.,1,.>) / solver 2                 7 / 7      19860 - 19958 / 19976 - 19991 0.04 - 0.70 %   exact
  mix2 (MIX 2) / general loop                   2 / 8      19863 - 19977                 0.11 - 0.69 %   exact
  counting builds                               13         as their launches             the same raw tallies; every counter inside its bounds
  path length (Flx_mhest = 1)                   6          19874 - 19977                 0.11 - 0.63 %   below 0.00 - 0.12, above 0.02 - 0.33
  Heat: every element a multiple of 0.5 bit for bit, except in the abst scene (97.1 % of them, the others 6.0e-8 relative off: HEAT_REL).
  E_emul of the path-length classes 0.3 - 2.3e-7, the allowance 4.8 - 9.3e-7 relative.

Mutations of scratch builds (profiles/r25/mutations.log; arithmetic only, indices kept in range), and the tests of the 101 that fail under each:
  the fold of a run record's crossing column shifted by one at the wrap (k_tl_runs)   6: default-to_top (both surfaces), -to_surface, -nz3_1 and
                                                                                      -none_varying over Lambert, path-to_surface: the launches
                                                                                      whose runs of three levels and more wrap in x
  plane 1 for plane 2 on the up leg (tbase and the run records' plane)                60: every flux-loop launch over the Lambert surface
  the heating cell taken after the face (block C: layer k + stepk)                    88: every flux-loop launch but none_varying (nothing is walked there)
  tz advanced by the layer just left (phase A)                                        27: every stacked launch of the flux loop -- the one scene
                                                                                      with walked layers on top of each other
  the reflected direction's sqrt(u2) replaced by u2 (block B5)                        60: every flux-loop launch over the Lambert surface
  px not re-based after an x wrap (fold_xy: clamped instead)                          83: the launches whose flights move in x under solvers 0 and 1, 7 of the general loop's among them
  The general loop's own copies of the first five were not mutated: its launches run the same predictions.
"""

import numpy as np
import pytest

from tests import flight_ref as F
from tests import readout_ref as rref

pytestmark = pytest.mark.gpu

HEAT_REL = 2.0**-22
COUNTING = ('default-base-lambert', 'default-stacked-black', 'no_runs-base', 'atomics-base', 'full_lists-base', 'small-base', 'tiles-base', 'solver1-base-lambert',
            'solver2-base-lambert', 'mix2-base', 'default-two-lambert', 'general-base-solver0', 'general-base-solver1')


def _run(solver, launch, sc, counting=False):
    """one launch: raw flux (3, nz + 1, ny, nx) and heat (nz, ny, nx) float64 through bound buffers, the read-outs, the route, the counters"""
    import torch
    dev = 'cuda:0'
    flux = torch.zeros(3*(sc.nz + 1)*sc.ny*sc.nx, dtype=torch.float64, device=dev)
    heat = torch.zeros(sc.nz*sc.ny*sc.nx, dtype=torch.float64, device=dev)
    out = {}
    try:
        solver.set_kernel(general=launch.general)
        solver.set_tuning(**{**F.TUNING_DEFAULTS, **dict(launch.tuning)})
        solver.load_scene(sc)
        solver.set_counting(counting)
        solver.bind(None, flux.data_ptr(), None, heat_ptr=heat.data_ptr())
        solver.reset()
        solver.run(launch.n, seed=launch.seed, offset=launch.offset); solver.sync()
        torch.cuda.synchronize()
        out['kernel'] = solver.kernel_name()
        out['flux'] = flux.cpu().numpy().reshape(3, sc.nz + 1, sc.ny, sc.nx).copy()
        out['heat'] = heat.cpu().numpy().reshape(sc.nz, sc.ny, sc.nx).copy()
        out['flux32'] = solver.flux(launch.n)
        out['heat32'] = solver.heating(launch.n)
        out['direct'] = solver.direct_levels()
        out['counters'] = solver.counters() if counting else None
    finally:
        solver.bind(None, None, None)
        solver.set_counting(False)
        solver.set_kernel(general=False)
        solver.set_tuning(**F.TUNING_DEFAULTS)
    return out


def _inside(name, what, raw, lo, hi):
    bad = (raw < lo) | (raw > hi)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError('%s: %s outside its bounds in %d elements of %d; first at %s: %r not in [%r, %r]; sum of raw - lower %.1f'
                             % (name, what, bad.sum(), bad.size, i, raw[i], lo[i], hi[i], float((raw - lo).sum())))


def _check_flux(launch, sc, p, got):
    """the flux planes, the totals, the analytic levels and the read-out of the flux"""
    name = launch.name
    raw = got['flux']
    lo, hi = p.gpu_flux()
    assert np.array_equal(raw*2.0, np.round(raw*2.0)), '%s: a flux tally is no multiple of 0.5' % name
    assert np.all(raw[hi == 0.0] == 0.0), '%s: a flux element no photon can touch holds %r' % (name, raw[hi == 0.0].max())
    _inside(name, 'flux', raw, lo, hi)
    albedo = F.ALBEDOS[launch.surface]
    into = raw[0, 0].sum()                                         # (level 0 lies below kdir in every scene: the direct beam is tallied there)
    assert p.kdir >= 1 and p.counts['surface'][0] <= into <= p.counts['surface'][1], (name, into, p.counts['surface'])
    if albedo > 0.0:
        assert raw[2, 0].sum() == albedo*into, (name, raw[2, 0].sum(), into)
        assert p.counts['top'][0] <= raw[2, sc.nz].sum()/albedo <= p.counts['top'][1], (name, raw[2, sc.nz].sum()/albedo, p.counts['top'])
    else:
        assert np.all(raw[2] == 0.0), name
    # ---- the read-out: amplitude x nx ny / N, plus the analytic direct beam at the levels >= kdir
    dl = got['direct']
    amp = float(dl[sc.nz])
    want_amp = rref.solar_amplitude(sc.src_flx, sc.src_the)
    assert abs(amp - want_amp) <= 2.0*np.spacing(want_amp), (name, amp, want_amp)
    ref_dl = F.direct_levels(sc)
    assert np.all(dl[:p.kdir] == 0.0) and np.all(np.abs(dl - amp*ref_dl) <= 1e-12*amp*ref_dl), (name, dl, amp*ref_dl)
    f32 = got['flux32']
    _inside(name, 'solver.flux', f32, rref.flux(lo, amp, dl, launch.n), rref.flux(hi, amp, dl, launch.n))
    return amp


def _check(launch, sc, p, got):
    """every assertion on a launch of the collision estimator; returns figures for the log"""
    name = launch.name
    amp = _check_flux(launch, sc, p, got)
    heat = got['heat']
    hlo, hhi = p.heat_lo*(1.0 - HEAT_REL), p.heat_hi*(1.0 + HEAT_REL)
    assert np.all(heat[p.heat_hi == 0.0] == 0.0), '%s: a heating cell no photon can collide in holds %r' % (name, heat[p.heat_hi == 0.0].max())
    _inside(name, 'heat', heat, hlo, hhi)
    near = np.round(heat*2.0)/2.0
    assert np.all(np.abs(heat - near) <= HEAT_REL*heat), '%s: a heating tally is no multiple of 0.5 to 2^-22' % name
    tot, ndrop = heat.sum(), int((p.drop != 0).sum())
    assert p.heat_lo.sum()*(1.0 - HEAT_REL) <= tot <= (p.heat_lo.sum() + ndrop)*(1.0 + HEAT_REL), (name, tot, p.heat_lo.sum(), ndrop)
    dz = np.diff(np.asarray(sc.zgrd, dtype=np.float64))
    _inside(name, 'solver.heating', got['heat32'], rref.heating(hlo, amp, dz, launch.n), rref.heating(hhi, amp, dz, launch.n))
    exact = float((heat == near).mean())
    print('%s [%s]: %d of %d photons compared (%.2f %% dropped), %d flux and %d heat elements, %d and %d of them non-zero; heat elements that are '
          'multiples of 0.5 bit for bit: %.1f %%, largest |heat - multiple| / heat %.2e (allowed %.2e)'
          % (name, got['kernel'], p.certain().sum(), launch.n, 100.0*p.dropped_share(), got['flux'].size, heat.size, (got['flux'] != 0).sum(), (heat != 0).sum(),
             100.0*exact, float(np.max(np.abs(heat - near)/np.where(heat > 0.0, heat, 1.0))), HEAT_REL))


def _check_counters(launch, sc, p, cnt):
    albedo = F.ALBEDOS[launch.surface]
    c = p.counts
    absorbed = (c['collide'][0] + (c['surface'][0] if albedo == 0.0 else 0), c['collide'][1] + (c['surface'][1] if albedo == 0.0 else 0))
    print('%s counters %s predicted %s absorbed %s' % (launch.name, {k: cnt[k] for k in ('photons', 'surface', 'escaped', 'absorbed', 'flux_tally', 'scatter', 'killed', 'roulette')}, c, absorbed))
    assert cnt['photons'] == launch.n and cnt['killed'] == 0 and cnt['roulette'] == 0, cnt
    assert c['surface'][0] <= cnt['surface'] <= c['surface'][1], (cnt['surface'], c['surface'])
    assert c['top'][0] <= cnt['escaped'] <= c['top'][1], (cnt['escaped'], c['top'])
    assert absorbed[0] <= cnt['absorbed'] <= absorbed[1], (cnt['absorbed'], absorbed)
    assert c['collide'][0] <= cnt['scatter'] <= c['collide'][1], (cnt['scatter'], c['collide'])
    assert cnt['absorbed'] + cnt['escaped'] == launch.n
    assert c['tally'][0] <= cnt['flux_tally'] <= c['tally'][1], (cnt['flux_tally'], c['tally'])


@pytest.mark.parametrize('launch', F.LAUNCHES, ids=F.LAUNCH_IDS)
def test_every_tally_against_float64(launch, solver):
    sc, p = F.evaluate(launch)
    got = _run(solver, launch, sc)
    _check(launch, sc, p, got)
    assert got['kernel'] == launch.kernel(), got['kernel']


@pytest.mark.parametrize('name', COUNTING)
def test_counting_builds_same_tallies_and_counters(name, solver):
    launch = F.LAUNCHES[F.LAUNCH_IDS.index(name)]
    sc, p = F.evaluate(launch)
    got = _run(solver, launch, sc, counting=True)
    _check(launch, sc, p, got)
    assert got['kernel'] == launch.kernel(counting=True), got['kernel']
    _check_counters(launch, sc, p, got['counters'])


@pytest.mark.parametrize('launch', F.HEST_LAUNCHES, ids=F.HEST_IDS)
def test_path_length_heating_against_float64(launch, solver):
    sc, p = F.evaluate(launch)
    got = _run(solver, launch, sc)
    _check_flux(launch, sc, p, got)
    E = F.path_scale(launch)
    rel = max(4.0*E, 8.0*F.EPS)
    heat, want, unc = got['heat'], p.path['sum'], p.path['unc']
    # every term is positive and the uncertain photons can only add: below, the certain photons' sum less the float32 allowance and nothing
    # else; above, that sum plus the allowance plus what the uncertain photons could leave in the cell
    low = np.where(want > 0.0, (want - heat)/np.where(want > 0.0, rel*want, 1.0), np.where(heat < 0.0, np.inf, 0.0))
    high = np.where(rel*want + unc > 0.0, (heat - want)/np.where(rel*want + unc > 0.0, rel*want + unc, 1.0), np.where(heat > 0.0, np.inf, 0.0))
    print('%s [%s]: %d of %d photons compared (%.2f %% dropped); E_emul %.2e, allowed %.2e relative; largest (ref - heat) / (allowed x ref) %.3f; '
          'largest (heat - ref) / (allowed x ref + uncertain share) %.3f; cells %d, %d of them non-zero'
          % (launch.name, got['kernel'], p.certain().sum(), launch.n, 100.0*p.dropped_share(), E, rel, low.max(), high.max(), heat.size, (heat != 0).sum()))
    assert low.max() <= 1.0, (launch.name, 'below the certain photons\' sum', np.unravel_index(int(np.argmax(low)), low.shape), float(low.max()))
    assert high.max() <= 1.0, (launch.name, 'above what the uncertain photons allow', np.unravel_index(int(np.argmax(high)), high.shape), float(high.max()))
    assert got['kernel'] == launch.kernel(), got['kernel']
