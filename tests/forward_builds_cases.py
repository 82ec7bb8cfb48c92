"""
The cases of tests/test_gpu_forward_builds.py, shared with tools/record_forward_golden.py, which records what a library computes for them.

One small cloud scene (NX x NY columns, NZ layers, NZ3 of them walked voxel by voxel, a Lambert surface, a little gas absorption) in as
many variants as the host has builds of the forward kernels to choose from (entry_build ... tl_scatter_build):

    constituents   'default' one Rayleigh 1-D and one Henyey-Greenstein 3-D constituent (MIX 0); 'two3d' a second 3-D one (MIX 1);
                   'two1d' a second 1-D one (MIX 2, no tables); 'tab3d' the 3-D constituent scatters by a table (MIX 2; MIX 3 in the column
                   view); 'tab3d_two3d' a table and a second 3-D constituent (MIX 2 with tables)
    nang           angles of that table: NANG_WIDE makes the staged table large enough for the column view's workgroups of 512 threads
                   (launch_column: 3 x LDS <= 160 KB < 6 x LDS), and is the most the table budget takes (fill_scene: 24 KB and the index)
    views          nadir alone (the column table), an oblique one beside it (event records and k_rays), cameras
    surface        Lambert, or LSRT (k_rays' heavy build)
    source         the sun, thermal emission, both
    solver         3-D, partial 3-D

and one large scene for the flux loop's tallies of more than 1024 bins (`big_flux`: the bins hold 2^14 tally cells each).

run_case records, for one case, a counting run (the first 14 counters: functions of the histories alone) and a run of the production
build (the raw float64 tallies through bound buffers, sparse where the tally is large), each with the name of the route and the form
of the entry records the last launch read.
"""

import numpy as np

from er3t_amd.scene import Scene, SOLVER_3D, SOLVER_P3D, TARGET_FLUX, TARGET_HEAT, TARGET_RADIANCE
from er3t_amd.solver import COUNTER_NAMES

SEED, ID0 = 41, 3
NX, NY, NZ, NZ3, IZ3L = 10, 8, 8, 4, 3
N_SORTED, N_SMALL = 20000, 3000          # (4096 photons and more than one tile: the launch is sorted, a flux job keeps record lists)
NANG, NANG_WIDE = 181, 2048
COUNTERS = tuple(COUNTER_NAMES[:14])     # photons ... absorbed; the sched_* and ticks_* behind them depend on scheduling
TUNING_DEFAULTS = dict(tile_cols=-1, entry_records=1, tally_lists=1, tally_runs=1)
F3, P3 = SOLVER_3D, SOLVER_P3D
RAD, FLX, HEAT = TARGET_RADIANCE, TARGET_FLUX, TARGET_FLUX | TARGET_HEAT
WL_THERMAL, WL_MIXED, FSOL = 11.0, 3.75, 10.0


def cloud(constituents='default', nang=NANG, solver=F3, target=RAD, oblique=False, lsrt=False, source='solar', hest=0, camera=False,
          nx=NX, ny=NY, nz=NZ, nz3=NZ3, iz3l=IZ3L):
    rng = np.random.default_rng(5)
    dz = 250.0
    zgrd = dz*np.arange(nz+1)
    shape = (nz3, ny, nx)
    ext = (rng.uniform(1.0e-3, 8.0e-3, shape)*(rng.random(shape) < 0.6)).astype(np.float32)
    extp, omgp, apfp = [ext], [np.full(shape, 0.98, dtype=np.float32)], [np.full(shape, 0.85, dtype=np.float32)]
    ext1d, omg1d, apf1d = [np.full(nz, 1.0e-4)], [np.ones(nz)], [-np.ones(nz)]
    ang = pha = None
    if constituents in ('tab3d', 'tab3d_two3d'):
        ang = np.linspace(0.0, 180.0, nang)
        g = 0.8
        pha = ((1.0-g*g)/(1.0+g*g-2.0*g*np.cos(np.deg2rad(ang)))**1.5)[None]
        apfp[0] = np.where(ext > 0.0, 1.0, -1.0).astype(np.float32)          # (a real 1-based table index; empty voxels: Rayleigh)
    if constituents in ('two3d', 'tab3d_two3d'):
        extp.append(np.full(shape, 1.0e-4, dtype=np.float32)); omgp.append(np.full(shape, 0.85, dtype=np.float32)); apfp.append(np.full(shape, 0.6, dtype=np.float32))
    if constituents == 'two1d':
        ext1d.append(np.full(nz, 5.0e-5)); omg1d.append(np.full(nz, 0.9)); apf1d.append(np.full(nz, 0.6))
    kw = dict(zgrd=zgrd, ext1d=np.stack(ext1d), omg1d=np.stack(omg1d), apf1d=np.stack(apf1d), abs1d=np.full(nz, 2.0e-5), nx=nx, ny=ny, dx=100.0, dy=120.0,
              nz3=nz3, iz3l=iz3l, extp=np.stack(extp), omgp=np.stack(omgp), apfp=np.stack(apfp), ang=ang, pha=pha,
              src_the=150.0, src_phi=250.0, src_qmax=0.0, solver=solver, target=target, heat_estimator=hest)
    if lsrt:
        psfc = np.zeros((5, ny, nx), dtype=np.float32)
        psfc[0], psfc[1], psfc[2] = 0.25, 0.03, 0.12
        kw.update(jsfc=np.full((ny, nx), 4.0, dtype=np.float32), psfc=psfc)
    else:
        kw.update(sfc_mtype=1, sfc_param=[0.2, 0, 0, 0, 0])
    if source != 'solar':
        kw.update(src_mtype=3 if source == 'thermal' else 2, src_wlen=WL_THERMAL if source == 'thermal' else WL_MIXED,
                  tmp1d=np.linspace(295.0, 275.0, nz+1), tmpa3d=rng.uniform(-4.0, 4.0, shape))
        if source == 'mixed':
            kw.update(src_fsol=FSOL)
    if camera:
        kw.update(rad_kind=1, view_the=[0.0, 180.0], view_phi=[0.0, 0.0], view_zloc=[100.0, 1900.0], cam_xpos=[0.3, 0.3], cam_ypos=[0.6, 0.6],
                  cam_psi=[0.0, 0.0], cam_qmax=[180.0, 180.0], cam_umax=[90.0, 90.0], cam_vmax=[180.0, 180.0], cam_apsize=[0.05, 0.05],
                  nxr=3, nyr=2, cam_mpmap=2, cam_mrproj=1)
    elif target & RAD:
        the, phi = ([180.0, 140.0], [0.0, 30.0]) if oblique else ([180.0], [0.0])
        kw.update(view_the=the, view_phi=phi, view_zloc=[705000.0]*len(the), nxr=nx, nyr=ny)
    return Scene(**kw)


def big_flux():
    """three layers, the middle one walked voxel by voxel, over so many columns that the flux tally has more than 1024 bins of 2^14 cells"""
    return cloud(target=FLX, nx=1200, ny=1190, nz=3, nz3=1, iz3l=2)


def _case(want, n=N_SORTED, general=False, tuning=None, form=None, **scene):
    """want: the route's name with %d for COUNT; form: the entry records of the last launch (None: not looked at)"""
    return dict(want=want, n=n, general=general, tuning=dict(tuning or {}), form=form, scene=scene)


FORM_NONE, FORM_LONG, FORM_SHORT = 0, 3, 2     # (mi3d_device.h: kEntryF4, kEntryF4Short -- float4 per block of 64 photons and part)

CASES = {}
# ---- the column loop: k_transport_lean<C,P,0,MIX>, its entry records and workgroups
CASES.update({
    'col_mix0_short':  _case('k_transport_lean<%d,0,0,0>', form=FORM_SHORT),
    'col_mix0_long':   _case('k_transport_lean<%d,0,0,0>', form=FORM_LONG, tuning=dict(entry_records=2)),
    'col_mix0_none':   _case('k_transport_lean<%d,0,0,0>', form=FORM_NONE, tuning=dict(entry_records=0)),
    'col_mix0_small':  _case('k_transport_lean<%d,0,0,0>', n=N_SMALL),
    'col_mix0_p3d':    _case('k_transport_lean<%d,1,0,0>', solver=P3, form=FORM_SHORT),
    'col_mix1':        _case('k_transport_lean<%d,0,0,1>', constituents='two3d', form=FORM_LONG),
    'col_mix2':        _case('k_transport_lean<%d,0,0,2>', constituents='two1d', form=FORM_LONG),
    'col_mix2_p3d':    _case('k_transport_lean<%d,1,0,2>', constituents='tab3d_two3d', solver=P3),
    'col_mix2_wide':   _case('k_transport_lean<%d,0,0,2>', constituents='tab3d_two3d', nang=NANG_WIDE),
    'col_mix3':        _case('k_transport_lean<%d,0,0,3>', constituents='tab3d'),
    'col_mix3_wide':   _case('k_transport_lean<%d,0,0,3>', constituents='tab3d', nang=NANG_WIDE),
})
# ---- event records and k_rays: the emit builds, the light, plain, heavy and camera builds of the ray kernel
CASES.update({
    'rays_mix0_plain': _case('k_transport_lean<%d,0,2,0> + k_rays', oblique=True),
    'rays_mix1_p3d':   _case('k_transport_lean<%d,1,2,1> + k_rays', oblique=True, constituents='two3d', solver=P3),
    'rays_mix2_tab':   _case('k_transport_lean<%d,0,2,2> + k_rays', oblique=True, constituents='tab3d'),
    'rays_heavy':      _case('k_transport_lean<%d,0,2,0> + k_rays', oblique=True, lsrt=True),
    'rays_heavy_p3d':  _case('k_transport_lean<%d,1,2,2> + k_rays', oblique=True, lsrt=True, constituents='two1d', solver=P3),
    'rays_camera':     _case('k_transport_lean<%d,0,2,0> + k_rays', camera=True),
    'rays_thermal':    _case('k_transport<%d,2,0,0> [thermal] + k_rays', camera=True, source='thermal'),
})
# ---- the general loop: k_transport<C,MARCHK,F,P,SRC>
for _p in (0, 1):
    for _m in (0, 1):
        for _f in (0, 1):
            CASES['gen_m%d_f%d_p%d' % (_m, _f, _p)] = _case('k_transport<%%d,%d,%d,%d>' % (_m, _f, _p), general=True, solver=P3 if _p else F3,
                                                            oblique=bool(_m), target=(RAD | FLX) if _f else RAD)
CASES.update({
    'gen_thermal_rad':  _case('k_transport<%d,1,0,0> [thermal]', oblique=True, source='thermal'),
    'gen_thermal_flux': _case('k_transport<%d,0,1,0> [thermal]', target=FLX, source='thermal'),
    'gen_mixed_rad':    _case('k_transport<%d,1,0,0> [solar+thermal]', oblique=True, source='mixed'),
    'gen_mixed_flux':   _case('k_transport<%d,0,1,1> [solar+thermal]', target=FLX, source='mixed', solver=P3),
})
# ---- the flux loop: k_transport_flux<C,P,MIX,HEST> and the sort of its records
_LISTS = ' + k_tl_scatter + k_tl_sum'
for _mix, _cons in enumerate(('default', 'two3d', 'tab3d')):
    for _h in (0, 1):
        for _p in (0, 1):
            CASES['flux_mix%d_h%d_p%d' % (_mix, _h, _p)] = _case('k_transport_flux<%%d,%d,%d%s>' % (_p, _mix, ',1' if _h else '') + _LISTS, constituents=_cons,
                                                                 target=HEAT if _h else FLX, hest=_h, solver=P3 if _p else F3)
CASES.update({
    'flux_small':    _case('k_transport_flux<%d,0,0>', target=FLX, n=N_SMALL),
    'flux_atomics':  _case('k_transport_flux<%d,0,0>', target=FLX, tuning=dict(tally_lists=0)),
    'flux_no_runs':  _case('k_transport_flux<%d,0,0>' + _LISTS, target=HEAT, tuning=dict(tally_runs=0)),
    'flux_hist_wg':  _case('k_transport_flux<%d,0,0>' + _LISTS, n=4100, tuning=dict(tile_cols=-1), big=True),
})


def make_scene(name):
    s = CASES[name]['scene']
    return big_flux() if s.get('big') else cloud(**s)


def tally_events(name, counters):
    """n of the bound n 2^-53: the tally events of the case's counting run that can enter an element of a raw tally"""
    c = dict(zip(COUNTERS, (int(v) for v in counters)))
    return c['le_column'] + c['le_rays'] + c['flux_tally']


def _sparse(t):
    """(indices, values) of the non-zero elements of a flat device tensor"""
    idx = t.nonzero().flatten()
    return idx.cpu().numpy().astype(np.int64), t[idx].cpu().numpy().copy()


def run_once(sol, name, counting, sc=None):
    """one run of a case: the route's name, the entry form, the counters (counting) or the raw tallies (not counting)"""
    import torch
    case = CASES[name]
    sc = sc if sc is not None else make_scene(name)
    n = case['n']
    dev = 'cuda:0'
    rad = torch.zeros(max(sc.nview*sc.nxr*sc.nyr, 1), dtype=torch.float64, device=dev) if sc.target & RAD else None
    flux = torch.zeros(3*(sc.nz+1)*sc.ny*sc.nx, dtype=torch.float64, device=dev) if sc.target & FLX else None
    heat = torch.zeros(sc.nz*sc.ny*sc.nx, dtype=torch.float64, device=dev) if sc.target & TARGET_HEAT else None
    out = {}
    try:
        sol.set_kernel(general=case['general'])
        sol.set_tuning(**{**TUNING_DEFAULTS, 'tile_cols': 4, **case['tuning']})
        sol.load_scene(sc)
        sol.set_counting(counting)
        sol.bind(rad.data_ptr() if rad is not None else None, flux.data_ptr() if flux is not None else None, None,
                 heat_ptr=heat.data_ptr() if heat is not None else None)
        sol.reset()
        sol.run(n, seed=SEED, offset=ID0); sol.sync()
        torch.cuda.synchronize()
        out['kernel'] = sol.kernel_name()
        try:
            out['form'] = int(sol.debug_entry()[0])
        except OSError:
            out['form'] = FORM_NONE
        if counting:
            c = sol.counters()
            out['counters'] = np.array([int(c[k]) for k in COUNTERS], dtype=np.int64)
        else:
            for key, t in (('rad', rad), ('flux', flux), ('heat', heat)):
                if t is None:
                    continue
                if t.numel() > 100000:
                    out[key+'_idx'], out[key+'_val'] = _sparse(t)
                    out[key+'_size'] = np.int64(t.numel())
                else:
                    out[key] = t.cpu().numpy().copy()
    finally:
        sol.bind(None, None, None)
        sol.set_counting(False)
        sol.set_kernel(general=False)
        sol.set_tuning(**TUNING_DEFAULTS)
    return out


def run_case(sol, name):
    """everything the fixture of a case holds, as a flat dict of arrays (what np.savez takes): run1_* counting, run0_* production"""
    sc = make_scene(name)
    out = {}
    for c in (1, 0):
        for k, v in run_once(sol, name, bool(c), sc).items():
            out['run%d_%s' % (c, k)] = np.asarray(v)
    return out


def tallies(r):
    """the raw tallies of a production run as {name: (indices or None, values, size)}: dense ones with indices None"""
    out = {}
    for key in ('rad', 'flux', 'heat'):
        if 'run0_'+key in r:
            out[key] = (None, np.asarray(r['run0_'+key]), int(np.asarray(r['run0_'+key]).size))
        elif 'run0_'+key+'_idx' in r:
            out[key] = (np.asarray(r['run0_'+key+'_idx']), np.asarray(r['run0_'+key+'_val']), int(r['run0_'+key+'_size']))
    return out


def largest_relative_difference(a, b):
    """between two production runs of a case, over the elements of every tally (zero against non-zero: inf)"""
    worst = 0.0
    ta, tb = tallies(a), tallies(b)
    for key in tb:
        ia, va, _ = ta[key]
        ib, vb, _ = tb[key]
        if ib is not None:
            if not np.array_equal(ia, ib):
                return float('inf')
        if np.any((va == 0.0) != (vb == 0.0)):
            return float('inf')
        nz = vb != 0.0
        if nz.any():
            worst = max(worst, float((np.abs(va[nz]-vb[nz])/np.abs(vb[nz])).max()))
    return worst
