"""
The local-estimate rays of the forward routes against float64, ray by ray (reference, prediction and scenes:
tests/le_rays_ref.py, held on the host by tests/test_le_rays_host.py).

Scenes in which nothing scatters and both ray roulettes are off: every photon makes at most one local estimate per view, from a point its
Philox blocks fix -- the surface point a solar photon reaches, the place a thermal photon is emitted at.  On 256 x 256 pixels the image is
a list of single rays, tau_gpu = -ln(image / (norm c)), and every launch asserts, for every ray that is not on the drop list:

  tau_ref <= 12     |tau_gpu - tau_ref| <= max(4 E_emul(class), (steps + 4) 2^-21): E_emul the largest distance of the float32 emulation of
                    the march from the reference over the class (scene, route, view), never anything the GPU gave; the second term is what
                    `steps` subtractions from the countdown 16 - rem round by, half an ulp of 16 each, and four more for the contribution,
                    the exponential and the float32 read-out.  Views answered from the column table (nadir, column_le on) the same with
                    steps = nz: k_build_column, tcol0 and tabove against float64
  tau_ref >= 16.1   the pixel is exactly 0 (the give-up); rays between 12 and 16.1 are not compared
  no ray predicted  the pixel is exactly 0, and the image's sum is the sum over the predicted pixels
  mi3d_last_kernel  the route the case is there for

Drop list (counted per launch; at most 10 % of the arriving rays, at least 1000 compared: the host module asserts both): a photon whose fate
-ln u against the sun path's optical depth is within 1e-4 relative of the threshold; a pixel coordinate within 1e-3 of a pixel edge; a
thermal CDF target within 1e-9 P_tot of a CDF entry (none occurs); a (view, pixel) shared with another arrival; and two of this module's:
an event within 1 mm of a sensor plane, and under solver != 0 an event within 1 mm of a column's face.

Routes x solvers 0, 1, 2 (free ray, column-bound ray): the default route with a Lambert surface (k_transport_lean<.,.,2,.> + k_rays, light
build), with an LSRT surface (R from tests/geometry_ref.py with the beam as incoming direction; the light build leaves those reflections to
the heavy one), set_kernel(general=True) (k_transport<.,1,0,.>), a nadir view alone (k_transport_lean<.,.,0,.>, the column table; and marched,
column_le off), the thermal general loop (k_transport<.,1,0,.> [thermal], up-looking views and downward rays too).  Every scene variant of
le_rays_ref.scene on the default route and the thermal loop; one launch with the sun at 40 degrees; one with counting on.

Measured on an MI355X (profiles/r23/le_rays.log), largest |tau_gpu - tau_ref| / bound per launch:
  route                                         launches                         largest ratio      dropped      compared per launch
  default, Lambert (lean<.,.,2,.> + k_rays)     solvers 0, 1, 2; column_le off   0.42 0.32 0.29; 0.34   0.7 - 2.4 %   4306 - 4818
  default, LSRT (heavy build)                   solvers 0, 1, 2                  0.42 0.33 0.28         0.7 - 2.4 %   4306 - 4818
  general loop, marched                         solvers 0, 1, 2; `two`, solver 1 0.32 0.12 0.12; 0.24   0.7 - 2.4 %   4306 - 4818
  nadir alone: column table / marched           solvers 0, 1, 2                  0.04 each              4.4 - 6.6 %   2205 - 2336
  thermal general loop                          solvers 0, 1, 2                  0.48 0.21 0.25         4.2 - 5.5 %   33183 - 34580
  scene variants, default route                 ten                              0.15 - 0.56            0.4 - 3.0 %   3012 - 6036
  scene variants, thermal loop                  ten                              0.26 - 0.73            4.2 - 4.6 %   33642 - 35476
  sun at 40 degrees, default route              one                              0.85                   1.5 %         5416
  The largest ratios belong to view 7, whose sensor lies exactly on the level between voxels and uniform layers: a ray that meets that level at
  a z face adds beta |zstop - z(t)| / |v_z| of one more layer, a rounding of z(t) = fma(v_z, t, z0) at t of some 1000 m.  Rays beyond 16.1
  (8 - 396 per launch, under solvers 1 and 2 only: no free ray of these scenes is that deep) leave their pixels exactly 0.  Nothing was
  found to fix: no kernel changed.

Mutations of a scratch build (profiles/r23/mutations.log; arithmetic only), and the tests that fail under each:
  the level crossing's tz advanced by the layer just left (k_rays)      default-stacked -- the one scene with walked layers on top of
                                                                        each other: elsewhere the ray leaves the walk at every level
  tup[] missing the starting layer's share (k_rays)                     every launch of the default route with a tail (20 tests)
  0 for dz where a ray comes down into the next layer (k_transport)     every thermal launch (13)
  tabove shifted by one layer (build_layers)                            37 of 42
  k_build_column: the depth above the bottom face                       every thermal launch and default-to_surface (14)
  the sensor plane of a view inside the atmosphere 0.1 % too high       36 of 42
  NOT caught, and not catchable: the sensor-plane test >= turned into > (k_rays and k_transport).  The step after the one that meets the
  plane at a face ends the ray with dtau = beta |zstop - z(t)| / |v_z| = 0: the mutant computes the same optical depth.  The mutation above it
  stands in for a ray that ends late at a sensor inside the atmosphere.
"""

import numpy as np
import pytest

from tests import le_rays_ref as L
from tests import readout_ref as rref

pytestmark = pytest.mark.gpu


def _launch(solver, case, sc, counting=False):
    try:
        solver.load_scene(sc, column_le=case.column_le)
        solver.set_kernel(general=(case.route == 'general'))
        solver.set_counting(counting)
        solver.reset()
        solver.run(case.n, seed=case.seed, offset=case.offset)
        img = solver.radiance(case.n)
        return img, solver.kernel_name(), (solver.counters() if counting else None)
    finally:
        solver.set_kernel()
        solver.set_counting(False)


def _norm(solver, case, sc):
    lx, ly = sc.nx*sc.dx, sc.ny*sc.dy
    if case.route == 'thermal':
        ptot, psol = solver.source_power()
        cdf = L.thermal_cdf(sc)
        dev_ptot, dev_cdf = solver.debug_thermal(cdf.size)
        # the prediction picks cells by its own float64 CDF: the device's must lie within the drop list's margin of it
        assert psol == 0.0 and dev_ptot == ptot and np.max(np.abs(dev_cdf - cdf)) <= L.CDF_MARGIN*cdf[-1], np.max(np.abs(dev_cdf - cdf))/cdf[-1]
        amp = rref.amplitude('thermal', sc.src_flx, ptot=ptot, lx=lx, ly=ly)
    else:
        amp = rref.solar_amplitude(sc.src_flx, sc.src_the)
    return rref.radiance_norm(amp, 'satellite', case.n, sc.nxr, sc.nyr)


def _check(case, sc, r, bound, img, norm):
    """every assertion on a launch's image; returns the largest |tau_gpu - tau_ref| / bound"""
    img = img.astype(np.float64)
    cmp_, dark = r.compared(), r.dark()
    pix = img[r.iv, r.jr, r.ir]
    assert np.all(pix[cmp_] > 0.0), 'a compared ray left its pixel empty: %d of %d' % ((pix[cmp_] <= 0.0).sum(), cmp_.sum())
    tau_gpu = -np.log(pix[cmp_]/(norm*r.c[cmp_]/r.absvz[cmp_]))
    err = np.abs(tau_gpu - r.tau[cmp_])
    ratio = err/bound[cmp_]
    worst = int(np.argmax(ratio))
    per_view = ' '.join('%d:%.2f' % (iv, ratio[r.iv[cmp_] == iv].max()) for iv in range(sc.nview) if np.any(r.iv[cmp_] == iv))
    print('%s [%s]: %d rays compared, %.1f %% of %d dropped, largest |tau_gpu - tau_ref| %.2e, largest ratio to the bound %.3f (view %d, tau %.2f); '
          'per view %s; %d rays beyond 16.1' % (case.name, case.kernel(), cmp_.sum(), 100.0*r.dropped_share(), r.m, err.max(), ratio[worst],
                                                r.iv[cmp_][worst], r.tau[cmp_][worst], per_view, dark.sum()))
    assert ratio[worst] <= 1.0, (case.name, int(r.iv[cmp_][worst]), float(r.tau[cmp_][worst]), float(tau_gpu[worst]), float(bound[cmp_][worst]))
    assert np.all(pix[dark] == 0.0), 'a ray beyond the cut-off reached its pixel'
    assert np.all(img[~r.maybe] == 0.0) and img.sum() == np.where(r.maybe, img, 0.0).sum()      # (the same order of summation)
    return float(ratio[worst])


@pytest.mark.parametrize('case', L.CASES, ids=L.CASE_IDS)
def test_every_ray_against_float64(case, solver):
    sc, r, te, st, bound, E = L.evaluate(case)
    img, name, _ = _launch(solver, case, sc)
    assert name == case.kernel(), name
    _check(case, sc, r, bound, img, _norm(solver, case, sc))


def test_counting_build_same_image_and_counters(solver):
    """the instrumented build of the default route: the image bit for bit, and the counters the prediction gives"""
    case = L.CASES[L.CASE_IDS.index('default-s0')]
    sc, r, te, st, bound, E = L.evaluate(case)
    img, name, _ = _launch(solver, case, sc)
    cimg, cname, cnt = _launch(solver, case, sc, counting=True)
    assert name == case.kernel() and cname == case.kernel(counting=True), (name, cname)
    assert np.array_equal(img.view(np.uint32), cimg.view(np.uint32))
    _check(case, sc, r, bound, cimg, _norm(solver, case, sc))
    column = np.array([case.column_le and L.column_view(sc, iv) for iv in range(sc.nview)])
    nv = sc.nview          # (every view of a solar case looks down from above the surface: one ray per view and arrival)
    want = {'surface': r.n_surface, 'le_rays': int(r.sure.sum()), 'le_column': int((r.sure & column[r.iv]).sum())}
    print('counters', {k: cnt[k] for k in ('photons', 'surface', 'le_rays', 'le_column', 'absorbed', 'escaped', 'killed')}, 'predicted', want,
          'photons on the fate margin', r.n_margin)
    assert want['le_rays'] == nv*r.n_surface and want['le_column'] == r.n_surface
    assert abs(cnt['surface'] - want['surface']) <= r.n_margin
    assert abs(cnt['le_rays'] - want['le_rays']) <= nv*r.n_margin and abs(cnt['le_column'] - want['le_column']) <= r.n_margin
    assert cnt['photons'] == case.n and cnt['absorbed'] + cnt['escaped'] == case.n
