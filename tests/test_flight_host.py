"""
The reference of tests/test_gpu_flight.py (tests/flight_ref.py) held on the host: against the CPU oracle, against its own float32
emulation, against closed forms, and to the caps its drop list must keep.  No GPU.

  oracle      same ids, flux and heating, every scene variant x solvers 0, 1, 2 x both surfaces at the slant sun, and the other suns of the
              GPU launches: un-normalised, every oracle tally is a multiple of 0.5 to 1e-6 and lies inside [lower, upper] of the prediction
              made with the oracle's own float64 directions (rounded = False); surface, escape and collision counts inside their bounds.
              This is what makes the reference independent of the kernels
  caps        per launch: at most 3 % dropped, at least 10000 of 20000 (2500 of 3000) compared; per scene at the vertical sun: between
              25 % and 75 % of the photons collide before the surface, and at least 3 levels are crossed per photon
  emulation   the float32 walk (flight_ref.flight_emul) over the certain photons of a class: no crossing changes its column, no collision its
              cell, no photon its fate; the largest displacement of a crossing point is at most m(t) / 4.  Measured: at most 0.03 m(t) (the
              grazing sun): M_SCALE = 2^-18 stands as derived, not widened
  budget      per photon, the weight deposited + absorbed by the surface + escaped is 1
  histories   hand-made rays in le_rays_ref.one_cell_scene and slab_scene against closed forms: a wrap in x, a wrap in y, a collision in the
              last voxel layer, a photon that reaches the surface, a reflected photon that escapes
"""

import numpy as np
import pytest

from tests import flight_ref as F
from tests import le_rays_ref as L

N = 20000
SUNS = [('base', F.VERTICAL), ('base', F.ALONG_X), ('base', F.ALONG_X_NEG0), ('base', F.ALONG_NEG_Y), ('base', F.GRAZING), ('stacked', F.VERTICAL),
        ('stacked', F.ALONG_X), ('stacked', F.ALONG_NEG_Y), ('stacked', F.GRAZING), ('diag', F.DIAGONAL)]
ORACLE_CASES = [(v, s, F.SLANT, surf) for v in L.VARIANTS for s in (0, 1, 2) for surf in ('black', 'lambert')] + \
               [(v, 0, sun, surf) for v, sun in SUNS for surf in ('black', 'lambert')] + [('base', 1, F.GRAZING, 'lambert'), ('base', 2, F.GRAZING, 'lambert')]


def _id(c):
    return '%s-s%d-sun%g_%s-%s' % (c[0], c[1], c[2][0], repr(c[2][1]), c[3])


@pytest.mark.parametrize('case', ORACLE_CASES, ids=_id)
def test_prediction_against_the_oracle(case, oracle, nthreads):
    variant, solver, sun, surface = case
    sc = F.scene(variant, solver, sun, surface)
    p = F.predict(sc, N, F.SEED, F.ID0, rounded=False)
    heat = np.zeros((sc.nz, sc.ny, sc.nx))
    _, flux, cnt = oracle.run_raw(sc, N, F.SEED, F.ID0, nthreads=nthreads, heat=heat)
    lo, hi = p.oracle_flux()
    for what, got, a, b in (('flux', flux, lo, hi), ('heat', heat, p.heat_lo, p.heat_hi)):
        assert np.all(np.abs(got*2.0 - np.round(got*2.0)) <= 2.0e-6), (what, 'not a multiple of 0.5')
        got = np.round(got*2.0)/2.0
        bad = (got < a) | (got > b)
        assert not bad.any(), (what, int(bad.sum()), [tuple(int(v[0]) for v in np.nonzero(bad))], float(got[bad][0]), float(a[bad][0]), float(b[bad][0]))
        assert np.all(got[b == 0.0] == 0.0), what
    c = p.counts
    assert c['surface'][0] <= int(cnt[4]) <= c['surface'][1], (int(cnt[4]), c['surface'])
    assert c['top'][0] <= int(cnt[12]) <= c['top'][1], (int(cnt[12]), c['top'])
    assert c['collide'][0] <= int(cnt[3]) <= c['collide'][1], (int(cnt[3]), c['collide'])
    # (the oracle tallies the launch's top level and every level of the direct beam: N more than the HIP path's count at most)
    assert p.dropped_share() <= F.DROP_CAP


@pytest.mark.parametrize('launch', F.LAUNCHES + F.HEST_LAUNCHES, ids=F.LAUNCH_IDS + F.HEST_IDS)
def test_caps_of_every_launch(launch):
    sc, p = F.evaluate(launch)
    print('%s: %.2f %% dropped, %d compared' % (launch.name, 100.0*p.dropped_share(), p.certain().sum()))
    assert p.dropped_share() <= F.DROP_CAP
    assert p.certain().sum() >= (10000 if launch.n == F.N_SORTED else 2500)
    assert launch.n in (F.N_SORTED, F.N_SMALL) and (sc.nx, sc.ny, sc.nz) in ((5, 4, 7), (1, 4, 7), (5, 1, 7))
    lo, hi = p.gpu_flux()
    assert np.all(lo <= hi) and np.all(p.heat_lo <= p.heat_hi) and np.all(lo[0, p.kdir:] == 0.0) and np.all(hi[1] == 0.0)


@pytest.mark.parametrize('surface', ('black', 'lambert'))
@pytest.mark.parametrize('variant', L.VARIANTS)
def test_scenes_collide_and_cross_enough(variant, surface):
    sc = F.scene(variant, 0, F.VERTICAL, surface)
    p = F.predict(sc, N, F.SEED, F.ID0)
    share, cross = float((p.fate[:, 0] == 0).mean()), float(p.ncross.mean())
    print('%s %s: %.1f %% collide before the surface, %.2f levels crossed per photon' % (variant, surface, 100.0*share, cross))
    assert 0.25 <= share <= 0.75 and cross >= 3.0


EMUL_CLASSES = [(v, 0, F.SLANT, 'lambert') for v in L.VARIANTS] + [(v, 0, sun, 'lambert') for v, sun in SUNS] + \
               [(v, s, F.SLANT, 'lambert') for v in ('base', 'stacked') for s in (1, 2)] + [('base', 1, F.GRAZING, 'lambert'), ('base', 2, F.GRAZING, 'lambert')]


@pytest.mark.parametrize('case', EMUL_CLASSES, ids=_id)
def test_float32_walk_keeps_every_certain_photon_in_place(case):
    variant, solver, sun, surface = case
    r = F._emul_class(variant, solver, sun, str(sun[1]), surface)
    print('%s: %d photons, %d moved, largest displacement of a crossing point %.4f m(t), E_emul %.2e (per term %.2e)' % (_id(case), r['photons'], r['moved'], r['disp'], r['E'], r['E_term']))
    assert r['photons'] >= 2500
    assert r['moved'] == 0
    assert r['disp'] <= 0.25


@pytest.mark.parametrize('surface', ('black', 'lambert'))
@pytest.mark.parametrize('solver', (0, 1, 2))
def test_every_photon_ends_somewhere(solver, surface):
    sc = F.scene('stacked', solver, F.SLANT, surface)
    p = F.predict(sc, N, F.SEED, F.ID0)
    assert np.array_equal(p.budget.sum(axis=1), np.ones(N))
    albedo = F.ALBEDOS[surface]
    ok = p.certain()
    assert p.heat_lo.sum() + (1.0 - albedo)*p.counts['surface'][0] + albedo*p.counts['top'][0] == float(ok.sum())
    # the launch's top level and the surface's tallies: one per certain photon, one per arrival
    assert p.flux_lo[0, sc.nz].sum() == float(ok.sum()) and p.flux_lo[2, 0].sum() == albedo*p.counts['surface'][0]
    assert p.flux_lo[0, 0].sum() == p.counts['surface'][0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# hand-made histories, closed forms
# ---------------------------------------------------------------------------------------------------------------------------------------
ZG = L.ZGRD
BETA = 2.0**-10


def _crossings(leg):
    c = leg.cross
    return list(zip(c['lev'].tolist(), c['iy'].tolist(), c['ix'].tolist()))


def test_history_wrap_in_x():
    """slab: from (590, 150) on the top along (sin 60, 0, -cos 60): x leaves the 600 m domain after 10 m and comes back in column 0"""
    sc = L.slab_scene(BETA)
    th = np.radians(60.0)
    d = np.array([np.sin(th), 0.0, -np.cos(th)])
    need = 0.5                              # path 0.5 / beta = 512 m: z = 1500 - 256 = 1244 (layer 5), x = 590 + 443.4 = 1033.4 -> 433.4 (column 3)
    leg = F.march(sc, [[590.0, 150.0, 1500.0]], d, need)
    assert leg.fate[0] == 0 and tuple(leg.cell[0]) == (5, 1, 3) and abs(leg.tend[0] - 512.0) < 1e-9
    # level 6 (z = 1250) at t = 500: x = 590 + 433.01 = 1023.01 -> 423.01: column 3, y stays in row 1
    assert _crossings(leg) == [(6, 1, 3)] and abs(leg.cross['t'][0] - 500.0) < 1e-9
    assert abs(np.mod(leg.cross['x'][0], 600.0) - (590.0 + 500.0*np.sin(th) - 600.0)) < 1e-9


def test_history_wrap_in_y():
    """slab: from (60, 10) along (0, -sin 45, -cos 45): y leaves the 400 m domain after 10 m and wraps three more times on the way down: level
    6 (250 m further) is crossed at y = -240 -> 160, row 1; to the surface through all seven levels"""
    sc = L.slab_scene(BETA)
    s = np.sqrt(0.5)
    leg = F.march(sc, [[60.0, 10.0, 1500.0]], [0.0, -s, -s], np.inf)
    assert leg.fate[0] == 1 and abs(leg.tend[0] - 1500.0/s) < 1e-9
    want = []
    for lev in range(6, -1, -1):
        y = np.mod(10.0 - (1500.0 - ZG[lev]), 400.0)
        want.append((lev, int(y//100.0), 0))
    assert _crossings(leg) == want and want[0] == (6, 1, 0) and want[-1] == (0, int(np.mod(10.0 - 1500.0, 400.0)//100.0), 0)


def test_history_collision_in_the_last_voxel_layer():
    """slab carried by voxels (layers 2 .. 4): a vertical photon with tau = beta (1500 - 500) collides at z = 500, inside layer 2, the lowest
    voxel layer; with tau = beta 1100 it has left the voxels and collides at z = 400 on the level below: the cell the direction points into"""
    sc = L.slab_scene(BETA, nz3=3)
    leg = F.march(sc, [[300.0, 250.0, 1500.0]]*2, [0.0, 0.0, -1.0], [BETA*1000.0, BETA*1100.0 + 1e-12])
    assert leg.fate.tolist() == [0, 0] and tuple(leg.cell[0]) == (2, 2, 2) and tuple(leg.cell[1]) == (1, 2, 2)
    assert np.array_equal(leg.cross['lev'][leg.cross['ph'] == 0], [6, 5, 4, 3]) and np.array_equal(leg.cross['lev'][leg.cross['ph'] == 1], [6, 5, 4, 3, 2])
    assert leg.drop[1] & F.D_FATE                       # (tau within 1e-4 of a face: on the drop list)


def test_history_reaches_the_surface():
    """one cloudy cell in a vacuum (column (2, 1) of layer 3, x 240..360, y 100..200, z 600..850): a vertical photon beside it reaches the
    surface whatever its free path; one through it with tau < beta 250 collides at z = 850 - tau / beta; with more it reaches the surface"""
    beta = 1.0/128.0
    sc = L.one_cell_scene(beta)
    leg = F.march(sc, [[100.0, 150.0, 1500.0], [300.0, 150.0, 1500.0], [300.0, 150.0, 1500.0]], [0.0, 0.0, -1.0], [1e-3, 1.0, 2.0])
    assert leg.fate.tolist() == [1, 0, 1]
    assert tuple(leg.cell[1]) == (3, 1, 2) and abs(leg.tend[1] - (650.0 + 128.0)) < 1e-9
    assert np.array_equal(leg.cross['lev'][leg.cross['ph'] == 0], [6, 5, 4, 3, 2, 1, 0]) and np.array_equal(leg.cross['lev'][leg.cross['ph'] == 1], [6, 5, 4])
    assert set(leg.cross['ix'][leg.cross['ph'] == 0].tolist()) == {0} and set(leg.cross['ix'][leg.cross['ph'] == 2].tolist()) == {2}


def test_history_reflected_photon_escapes():
    """the same cell from below: a photon reflected at (300, 250) into (0, -sin 30, cos 30) enters the cell's column at y = 200, z = 86.6 and
    leaves its row at y = 100, z = 259.8, far below the cell: it escapes through the top, crossing levels 1 .. 7; every column closed form"""
    sc = L.one_cell_scene(1.0/128.0)
    th = np.radians(30.0)
    d = np.array([0.0, -np.sin(th), np.cos(th)])
    leg = F.march(sc, [[300.0, 250.0, 0.0]], d, 5.0, grow=F.ROT_GROW)
    assert leg.fate[0] == 2 and abs(leg.tend[0] - 1500.0/np.cos(th)) < 1e-9 and leg.drop[0] == 0
    want = [(lev, int(np.mod(250.0 - np.tan(th)*ZG[lev], 400.0)//100.0), 2) for lev in range(1, 8)]
    assert _crossings(leg) == want
    # the same ray bound to its column (solvers 1 and 2): every level in column (2, 2)
    leg = F.march(sc, [[300.0, 250.0, 0.0]], d, 5.0, column=True)
    assert leg.fate[0] == 2 and _crossings(leg) == [(lev, 2, 2) for lev in range(1, 8)]
    # ... and through the cell: straight up under it, tau = 1 < 250 / 128: a collision at z = 600 + 128
    leg = F.march(sc, [[300.0, 150.0, 0.0]], [0.0, 0.0, 1.0], 1.0)
    assert leg.fate[0] == 0 and tuple(leg.cell[0]) == (3, 1, 2) and abs(leg.tend[0] - 728.0) < 1e-9


def test_kdir_and_the_analytic_levels():
    want = {'base': 5, 'to_surface': 3, 'to_top': 7, 'nz3_1': 3, 'none_varying': 2, 'stacked': 5}
    for variant, kd in want.items():
        sc = F.scene(variant, 0, F.SLANT)
        assert F.kdir_of(sc) == kd, variant
        dl = F.direct_levels(sc)
        assert dl[sc.nz] == 1.0 and np.all(dl[:kd] == 0.0) and np.all(np.diff(dl[kd:]) >= 0.0) and np.all(dl[kd:] > 0.0)
    # base: above level 5 the 1-D layers 5 and 6 with 5 and 10 units of 2^-15 / m over 250 m each, at mu0 = cos 30
    sc = F.scene('base', 0, F.SLANT)
    assert abs(F.direct_levels(sc)[5] - np.exp(-(5.0 + 10.0)*2.0**-15*250.0/np.cos(np.radians(30.0)))) < 1e-15
