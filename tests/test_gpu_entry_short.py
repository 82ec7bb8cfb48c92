"""
Short entry records (mi3d_device.h: kEntryF4Short) and the photon order of round 11.

k_entry writes what a new photon is where its first voxel walk begins.  For a solar source without a cone that shines from above, the
direction is the launch's and pz the thickness of the layer the photon stands in: the short form leaves the four words out (32 bytes
instead of 48) and the loop's build that reads it (k_transport_lean<., ., 0, 0, 256, 2>) takes them from its tables in LDS.
mi3d_set_tuning "entry_records": 0 none, 1 short where allowed (default), 2 long always; mi3d_debug_entry reports the form of the last
launch and copies its records out.

Scenes: a grid of 12 x 10 columns, six voxel layers (30 % of the voxels clear), three horizontally uniform layers above them, thick
enough (optical depth 0.39 along the beam) that a third of the first flights end up there -- records handed over in mode M_UNIF at the top
of the atmosphere -- while the others cross them (M_FLY, ran = 1).  Sun at 30 degrees, Lambert surface 0.3, nadir view.

Bounds.  The records: raw 32-bit words, equal.  Same ids and seed through the three settings are the same histories: event counters
equal as integers; the images differ by the order of their float32 partial sums only (tally window, pending register): 2e-5 of the
brightest pixel, the bound tests/test_gpu_parity.py holds the tally-window tests to for the same situation.

A thermal job never had entry records (its photons start anywhere, the general loop launches them), nor has a solar+thermal one: for
them the hook reports that there are none, MI3D_ESTATE, under either setting -- which is what "not the short form" means there.

The photon order: the same permutation whenever the same launch is sorted, and a launch of 3.6e7 photons, the smallest kind at which a
block of k_bin_scatter sorts more than one chunk (4096 blocks x 8192 indices = 2^25).
"""

import math

import numpy as np
import pytest

from er3t_amd.scene import Scene, TARGET_FLUX, TARGET_RADIANCE, SOLVER_3D, SOLVER_P3D, SOLVER_IPA

pytestmark = pytest.mark.gpu

NX, NY, NZ3 = 12, 10, 6
FORM_SHORT, FORM_LONG = 2, 3
COUNTERS = ('photons', 'scatter', 'surface', 'killed', 'escaped', 'absorbed', 'roulette', 'steps3d', 'le_rays')


def entry_scene(solver=SOLVER_3D, above=3, cloud=True, qmax=0.0, target=TARGET_RADIANCE):
    nz = NZ3 + above
    rng = np.random.default_rng(11)
    zgrd = np.concatenate([250.0*np.arange(NZ3+1), 250.0*NZ3 + 1000.0*np.arange(1, above+1)])
    ext1d = np.full((1, nz), 2.0e-5); ext1d[0, NZ3:] = 1.5e-4
    shape = (NZ3, NY, NX)
    ext = (rng.uniform(2.0e-3, 2.0e-2, shape)*(rng.random(shape) < 0.7)).astype(np.float32) if cloud else np.zeros(shape, dtype=np.float32)
    kw = dict(zgrd=zgrd, ext1d=ext1d, omg1d=np.ones((1, nz)), apf1d=-np.ones((1, nz)), abs1d=np.zeros(nz), nx=NX, ny=NY, dx=100.0, dy=100.0,
              nz3=NZ3, iz3l=1, extp=ext[None], omgp=np.full((1,)+shape, 0.97, dtype=np.float32), apfp=np.full((1,)+shape, 0.85, dtype=np.float32),
              sfc_mtype=1, sfc_param=[0.3, 0, 0, 0, 0], src_the=150.0, src_phi=270.0, src_qmax=qmax, solver=solver, target=target)
    if target & TARGET_RADIANCE:
        kw.update(view_the=[180.0], view_phi=[0.0], view_zloc=[705000.0], nxr=NX, nyr=NY)
    return Scene(**kw)


def _mode_names(solver=None):
    """the lane modes of the kernels, by name (the enum of mi3d_kernels.hip), so that the test reads the records as the loop does"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'er3t_amd', 'csrc', 'mi3d_kernels.hip')).read()
    names = {n: int(v) for n, v in re.findall(r'\b(M_FLY|M_UNIF)\s*=\s*(\d+)\s*,', src)}
    assert set(names) == {'M_FLY', 'M_UNIF'} and names['M_FLY'] != names['M_UNIF'], 'the mode enum of mi3d_kernels.hip is not where this test reads it: %r' % names
    return names


def _records(solver, sc, n, setting, seed=3):
    """(form, fields by photon index of the launch) of one launch of n photons under "entry_records" = setting"""
    solver.set_tuning(tile_cols=4, entry_records=setting)
    solver.bind(None, None, None)
    solver.load_scene(sc); solver.set_counting(False); solver.reset()
    solver.run(n, seed=seed); solver.sync()
    assert solver.kernel_name().startswith('k_transport_lean<0,0,0,0>'), solver.kernel_name()
    form, rec = solver.debug_entry(n)
    rec = rec.view(np.uint32)                                   # [blocks of 64, part, 64, 4] raw words
    part = lambda p, c: rec[:, p, :, c].reshape(-1)[:n]
    if form == FORM_LONG:
        f = dict(px=part(0, 0), py=part(0, 1), pz=part(0, 2), rem=part(0, 3), ux=part(1, 0), uy=part(1, 1), uz=part(1, 2), r1=part(1, 3),
                 r2=part(2, 0), r3=part(2, 1), cell=part(2, 2), km=part(2, 3))
    else:
        f = dict(px=part(0, 0), py=part(0, 1), rem=part(0, 2), r1=part(0, 3), r2=part(1, 0), r3=part(1, 1), cell=part(1, 2), km=part(1, 3))
    # the records lie in the launch's order: by photon index of the launch through the order where the launch was sorted
    if n >= 4096:
        order, _ = solver.debug_order(n)
        assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
        f = {k: v[np.argsort(order, kind='stable')] for k, v in f.items()}
    return form, f


@pytest.mark.parametrize('n', [1, 63, 65, 4096 + 37, 100037])
def test_short_records_equal_the_long_ones_bit_for_bit(solver, n):
    sc = entry_scene()
    try:
        form_l, L = _records(solver, sc, n, 2)
        form_s, S = _records(solver, sc, n, 1)
    finally:
        solver.set_tuning(tile_cols=-1, entry_records=1)
    assert form_l == FORM_LONG and form_s == FORM_SHORT, (form_l, form_s)
    for k in S:
        assert np.array_equal(S[k], L[k]), (k, int((S[k] != L[k]).sum()))
    # what the short form leaves out is what the loop's tables give: the source direction and the thickness of the photon's layer
    th, ph = math.radians(sc.src_the), math.radians(sc.src_phi)
    sd = np.array([math.sin(th)*math.cos(ph), math.sin(th)*math.sin(ph), math.cos(th)], dtype=np.float32)
    for q, name in enumerate(('ux', 'uy', 'uz')):
        assert np.all(L[name].view(np.float32) == sd[q]), name
    k = (L['km'] & 0xffff).astype(np.int64)
    dz = np.diff(np.asarray(sc.zgrd, dtype=np.float64)).astype(np.float32)
    assert k.min() >= 0 and k.max() < sc.nz
    assert np.array_equal(L['pz'].view(np.float32), dz[k])
    # and the scene does what it is for: both kinds of record
    M = _mode_names(solver)
    mode = (L['km'] >> 16) & 0x7fff
    ran = L['km'] >> 31
    assert np.all((mode == M['M_FLY']) | (mode == M['M_UNIF']))
    assert np.all(k[mode == M['M_UNIF']] == sc.nz-1) and np.all(ran[mode == M['M_UNIF']] == 0)
    assert np.all(k[mode == M['M_FLY']] == NZ3-1) and np.all(ran[mode == M['M_FLY']] == 1)
    if n >= 4096:
        assert 0.2*n < (mode == M['M_UNIF']).sum() < 0.5*n


def _run(solver, sc, n, setting, counting, seed=9):
    solver.set_tuning(tile_cols=4, entry_records=setting)
    solver.bind(None, None, None)
    solver.load_scene(sc); solver.set_counting(counting); solver.reset()
    solver.run(n, seed=seed); solver.sync()
    out = {'counters': solver.counters(), 'kernel': solver.kernel_name()}
    try:
        out['form'] = solver.debug_entry()[0]
    except OSError:
        out['form'] = 0
    if sc.target & TARGET_RADIANCE:
        out['rad'] = solver.radiance(n).astype(np.float64)
    if sc.target & TARGET_FLUX:
        out['flux'] = solver.flux(n).astype(np.float64)
    return out


def _same_results(a, b, what):
    for k in COUNTERS:
        assert a['counters'][k] == b['counters'][k], (what, k, a['counters'][k], b['counters'][k])
    for key in ('rad', 'flux'):
        if key in a:
            print('%s: %s largest difference %.3e of the largest value' % (what, key, np.abs(a[key]-b[key]).max()/np.abs(b[key]).max()))
            assert np.abs(a[key]-b[key]).max() <= 2e-5*np.abs(b[key]).max(), (what, key)


SCENES = {'3d': dict(), 'ipa': dict(solver=SOLVER_IPA), 'p3d': dict(solver=SOLVER_P3D), 'no_layer_above': dict(above=0), 'cloud_free': dict(cloud=False)}


@pytest.mark.parametrize('counting', [True, False])
@pytest.mark.parametrize('name', list(SCENES))
def test_same_histories_through_every_setting(solver, name, counting):
    sc = entry_scene(**SCENES[name])
    n = 200000
    try:
        res = {s: _run(solver, sc, n, s, counting) for s in (0, 1, 2)}
    finally:
        solver.set_tuning(tile_cols=-1, entry_records=1)
    assert [res[s]['form'] for s in (0, 1, 2)] == [0, FORM_SHORT, FORM_LONG]
    p3d = 1 if name == 'p3d' else 0
    for s in (0, 1, 2):
        assert res[s]['kernel'].startswith('k_transport_lean<%d,%d,0,0>' % (1 if counting else 0, p3d)), res[s]['kernel']
        assert res[s]['counters']['photons'] == n
    if counting:
        c = res[2]['counters']
        assert c['scatter'] > 0 and c['killed'] + c['escaped'] + c['absorbed'] == n
    _same_results(res[1], res[2], name + ': short against long')
    _same_results(res[1], res[0], name + ': short against none')


def test_records_of_the_other_scenes(solver):
    """no uniform layer above the clouds: every record in mode M_FLY with ran = 0; no cloud: no layer is walked voxel by voxel (a voxel
    layer whose extinction does not vary is a uniform one, mi3d_api.hip: the layer table), the whole column is one run of uniform layers with
    nothing below it to fly into, and every record is handed over as it stands at the top of the atmosphere: M_UNIF, ran = 0, k = nz - 1"""
    M = _mode_names(solver)
    nz = NZ3 + 3
    try:
        _, a = _records(solver, entry_scene(above=0), 5000, 1)
        _, b = _records(solver, entry_scene(cloud=False), 5000, 1)
    finally:
        solver.set_tuning(tile_cols=-1, entry_records=1)
    assert np.all(((a['km'] >> 16) & 0x7fff) == M['M_FLY']) and np.all((a['km'] >> 31) == 0)
    assert np.all((a['km'] & 0xffff) == NZ3-1)
    assert np.all(((b['km'] >> 16) & 0x7fff) == M['M_UNIF']) and np.all((b['km'] >> 31) == 0) and np.all((b['km'] & 0xffff) == nz-1)


@pytest.mark.parametrize('case', ['cone', 'flux', 'thermal', 'solar_thermal'])
def test_where_the_short_form_must_not_be_used(solver, case):
    if case == 'cone':
        sc, want = entry_scene(qmax=0.533133), FORM_LONG
    elif case == 'flux':
        sc, want = entry_scene(target=TARGET_FLUX), FORM_LONG
    else:
        import dataclasses
        from tests.util import thermal_mixed_scene
        sc, want = thermal_mixed_scene(), 0                    # (no entry records at all: the hook says so)
        if case == 'solar_thermal':                            # (Src_mtype=2: its photons start anywhere too, the general loop launches them)
            sc = dataclasses.replace(sc, src_mtype=2, src_fsol=5.0, src_the=150.0)
    n = 200000
    try:
        a = _run(solver, sc, n, 1, True)
        b = _run(solver, sc, n, 2, True)
    finally:
        solver.set_tuning(tile_cols=-1, entry_records=1)
    assert a['form'] == want and b['form'] == want, (case, a['form'], b['form'], a['kernel'])
    assert a['form'] != FORM_SHORT
    _same_results(a, b, case)


def test_photon_order_is_the_same_permutation_every_time(solver, oracle):
    """mi3d_debug_order on 100 037 photons over 3 x 3 tiles: a permutation of the launch's indices grouped by tile, the tiles' ends at the
    cursors, every index in the piece of the tile its photon starts above (the property test_photon_order_is_a_permutation_grouped_by_tile
    holds) -- and the same order when the same launch is sorted again: the sort takes no atomic on global memory."""
    sc = entry_scene()
    n, tc, seed = 100037, 4, 77
    got = []
    try:
        solver.set_tuning(tile_cols=tc)
        solver.bind(None, None, None)
        solver.load_scene(sc); solver.set_counting(True)
        for rep in range(2):
            solver.reset(); solver.run(n, seed=seed); solver.sync()
            assert solver.counters()['photons'] == n
            got.append(solver.debug_order(n))
    finally:
        solver.set_tuning(tile_cols=-1)
    order, tend = got[0]
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
    ntx, nty = (sc.nx+tc-1)//tc, (sc.ny+tc-1)//tc
    assert (ntx, nty) == (3, 3)
    ends = tend[:ntx*nty].astype(np.int64)
    assert np.all(np.diff(ends) >= 0) and ends[-1] == n
    starts = np.concatenate(([0], ends[:-1]))
    # the tile of every index from the launch position of its photon (Philox block 0 of the oracle)
    rng = np.random.default_rng(5)
    for pos in rng.integers(0, n, size=300):
        w = oracle.philox(seed, int(order[pos]), 0)
        u = ((w >> 9).astype(np.float64) + 0.5)/8388608.0
        x, y = np.float32(u[0])*np.float32(sc.dx*sc.nx), np.float32(u[1])*np.float32(sc.dy*sc.ny)
        tx, ty = min(int(x/(sc.dx*tc)), ntx-1), min(int(y/(sc.dy*tc)), nty-1)
        t = ty*ntx + (ntx-1-tx if ty & 1 else tx)
        # (a position on a tile's edge may round either way in float32: the neighbouring tile is as good)
        near = [tt for tt in (t-1, t, t+1) if 0 <= tt < ntx*nty and starts[tt] <= pos < ends[tt]]
        assert near, (pos, t)
        assert near[0] == t or abs(x/(sc.dx*tc) - round(x/(sc.dx*tc))) < 1e-3 or abs(y/(sc.dy*tc) - round(y/(sc.dy*tc))) < 1e-3, (pos, t, near)
    assert np.array_equal(got[1][0], order) and np.array_equal(got[1][1][:ntx*nty], tend[:ntx*nty])


def test_photon_order_of_a_launch_with_more_than_one_chunk_per_block(solver, oracle):
    """k_bin_scatter sorts 8192 indices a chunk, and a block has more than one chunk only above 4096 x 8192 = 2^25 indices a launch.
    36 000 037 indices give every block a slab of 8792: one full chunk and one of 600, so the tiles' places are carried from chunk to
    chunk, the waves' counters are used a second time, and the last block's slab is cut short by the launch's end.  Asked: a permutation;
    the tiles' ends ascending and the last the launch's size; every piece its tile's share of the launch; sampled indices in the piece of
    the tile their photon starts above; and inside a piece the indices in the order of their (block, chunk), which is how the places are
    handed out."""
    sc = entry_scene()
    n, tc, seed = 36000037, 4, 5
    try:
        solver.set_tuning(tile_cols=tc)
        solver.bind(None, None, None)
        solver.load_scene(sc); solver.set_counting(False); solver.reset()
        solver.run(n, seed=seed); solver.sync()
        order, tend = solver.debug_order(n)
    finally:
        solver.set_tuning(tile_cols=-1)
    assert order.shape == (n,) and int(order.max()) == n-1
    assert np.all(np.bincount(order, minlength=n) == 1)
    ntx, nty = 3, 3
    ends = tend[:ntx*nty].astype(np.int64)
    assert np.all(np.diff(ends) > 0) and ends[-1] == n
    starts = np.concatenate(([0], ends[:-1]))
    # the photons start uniformly over 12 x 10 columns in tiles of 4 x 4, the last row of tiles two columns deep: a piece's share of the
    # launch has a standard deviation of 6e-5 of the launch; 1e-3 is seventeen of them and a fraction of one block's slabs
    share = np.array([16, 16, 16, 16, 16, 16, 8, 8, 8], dtype=np.float64)/120.0
    assert np.all(np.abs((ends-starts)/n - share) < 1e-3)
    rng = np.random.default_rng(6)
    for pos in rng.integers(0, n, size=200):
        w = oracle.philox(seed, int(order[pos]), 0)
        u = ((w >> 9).astype(np.float64) + 0.5)/8388608.0
        x, y = np.float32(u[0])*np.float32(sc.dx*sc.nx), np.float32(u[1])*np.float32(sc.dy*sc.ny)
        tx, ty = min(int(x/(sc.dx*tc)), ntx-1), min(int(y/(sc.dy*tc)), nty-1)
        t = ty*ntx + (ntx-1-tx if ty & 1 else tx)
        on_edge = abs(x/(sc.dx*tc) - round(x/(sc.dx*tc))) < 1e-3 or abs(y/(sc.dy*tc) - round(y/(sc.dy*tc))) < 1e-3
        assert starts[t] <= pos < ends[t] or on_edge, (pos, t)
    slab = ((n + 4095)//4096 + 7)//8*8
    assert slab == 8792
    idx = order.astype(np.int64)
    chunk = (idx//slab)*2 + (idx % slab)//8192
    for s, e in zip(starts, ends):
        assert np.all(np.diff(chunk[s:e]) >= 0)
