"""
ctypes binding of libmi3drt.so (C-ABI: include/mi3d.h) and a small object wrapper.

This is the in-process replacement of the reference's process boundary
`os.system('<MCARATS_V010_EXE> <Nphoton> <solver> <inp> <out>')` (er3t/rtm/mca/mca_run.py:101-115,
179-181).  There is no CPU fallback: if the shared library is missing or no GPU is visible every
compute call raises OSError.
"""

import ctypes as C
import os

import numpy as np

from .scene import Scene, TARGET_FLUX, TARGET_RADIANCE, TARGET_HEAT

__all__ = ['Mi3dSolver', 'load_library', 'library_path', 'COUNTER_NAMES']

MAX_VIEW = 16
NCOUNTER = 24
COUNTER_NAMES = ['photons', 'steps', 'steps3d', 'scatter', 'surface', 'le_rays', 'le_steps', 'le_steps3d',
                 'le_column', 'flux_tally', 'roulette', 'killed', 'escaped', 'absorbed',
                 'sched_a_lanes', 'sched_a_slots', 'sched_b_lanes', 'sched_b_slots',
                 'ticks_a', 'ticks_b0', 'ticks_b12', 'ticks_b34', 'ticks_b5', 'ticks_b6']

_fp  = C.POINTER(C.c_float)
_dp  = C.POINTER(C.c_double)
_u64 = C.c_uint64
_LIB = None

# every symbol include/mi3d.h declares: (name, restype, argtypes)
_SIGNATURES = [
    ('mi3d_version'            , C.c_int   , []),
    ('mi3d_last_error'         , C.c_char_p, []),
    ('mi3d_device_count'       , C.c_int   , []),
    ('mi3d_create'             , C.c_int   , [C.c_int, C.POINTER(C.c_void_p)]),
    ('mi3d_destroy'            , C.c_int   , [C.c_void_p]),
    ('mi3d_set_atm1d'          , C.c_int   , [C.c_void_p, C.c_int, _dp, C.c_int, _fp, _fp, _fp, _fp]),
    ('mi3d_set_atm3d'          , C.c_int   , [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _fp, _fp, _fp, _fp]),
    ('mi3d_set_phase'          , C.c_int   , [C.c_void_p, C.c_int, C.c_int, _fp, _fp]),
    ('mi3d_set_surface'        , C.c_int   , [C.c_void_p, C.c_int, _fp]),
    ('mi3d_set_surface2d'      , C.c_int   , [C.c_void_p, C.c_int, C.c_int, _fp, _fp, _fp]),
    ('mi3d_set_source'         , C.c_int   , [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]),
    ('mi3d_set_thermal'        , C.c_int   , [C.c_void_p, C.c_int, C.c_double, C.c_int, _fp, _fp, _fp]),
    ('mi3d_set_solar_irradiance', C.c_int  , [C.c_void_p, C.c_double]),
    ('mi3d_get_source_power'   , C.c_int   , [C.c_void_p, _dp, _dp]),
    ('mi3d_set_views'          , C.c_int   , [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int]),
    ('mi3d_set_cameras'        , C.c_int   , [C.c_void_p, C.c_int] + [_dp]*10 + [C.c_int, C.c_int]),
    ('mi3d_set_camera_map'     , C.c_int   , [C.c_void_p, C.c_int, C.c_int]),
    ('mi3d_set_camera_method'  , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_set_view_method'    , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_set_emission_weights', C.c_int  , [C.c_void_p, C.c_int]),
    ('mi3d_bind_weights_buffer', C.c_int   , [C.c_void_p, C.c_void_p]),
    ('mi3d_get_emission_weights', C.c_int  , [C.c_void_p, _u64, _fp, _fp]),
    ('mi3d_debug_weights_staged', C.c_int  , [C.c_void_p]),
    ('mi3d_set_view_profiles'  , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_bind_view_profiles_buffer', C.c_int, [C.c_void_p, C.c_void_p]),
    ('mi3d_get_view_profiles'  , C.c_int   , [C.c_void_p, _u64, _fp, _fp]),
    ('mi3d_set_pixel_errors'   , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_bind_pixel_errors_buffer', C.c_int, [C.c_void_p, C.c_void_p]),
    ('mi3d_get_radiance_se'    , C.c_int   , [C.c_void_p, _u64, _fp]),
    ('mi3d_debug_backward_chunk', C.c_int  , [C.c_void_p]),
    ('mi3d_set_view_sunlight'  , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_set_view_columns'   , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_set_options'        , C.c_int   , [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]),
    ('mi3d_set_le_roulette'    , C.c_int   , [C.c_void_p, C.c_double]),
    ('mi3d_set_le_weight_roulette', C.c_int, [C.c_void_p, C.c_double]),
    ('mi3d_set_counting'       , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_bind_device_buffers', C.c_int   , [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('mi3d_bind_heating_buffer', C.c_int   , [C.c_void_p, C.c_void_p]),
    ('mi3d_set_heating_estimator', C.c_int , [C.c_void_p, C.c_int]),
    ('mi3d_prepare'            , C.c_int   , [C.c_void_p]),
    ('mi3d_reset'              , C.c_int   , [C.c_void_p]),
    ('mi3d_run'                , C.c_int   , [C.c_void_p, _u64, _u64, _u64]),
    ('mi3d_sync'               , C.c_int   , [C.c_void_p]),
    ('mi3d_last_kernel'        , C.c_char_p, [C.c_void_p]),
    ('mi3d_set_kernel'         , C.c_int   , [C.c_void_p, C.c_int]),
    ('mi3d_set_tuning'         , C.c_int   , [C.c_void_p, C.c_char_p, C.c_int]),
    ('mi3d_get_timing'         , C.c_int   , [C.c_void_p, _dp, C.POINTER(_u64)]),
    ('mi3d_get_radiance'       , C.c_int   , [C.c_void_p, _u64, _fp]),
    ('mi3d_get_flux'           , C.c_int   , [C.c_void_p, _u64, _fp]),
    ('mi3d_get_direct_levels'  , C.c_int   , [C.c_void_p, _dp]),
    ('mi3d_get_camera_direct'  , C.c_int   , [C.c_void_p, _dp]),
    ('mi3d_get_heating'        , C.c_int   , [C.c_void_p, _u64, _fp]),
    ('mi3d_get_emission'       , C.c_int   , [C.c_void_p, _fp]),
    ('mi3d_get_counters'       , C.c_int   , [C.c_void_p, C.POINTER(_u64)]),
    ('mi3d_stats_begin'        , C.c_int   , [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('mi3d_stats_set_analytic_share', C.c_int, [C.c_void_p, C.c_double]),
    ('mi3d_stats_add'          , C.c_int   , [C.c_void_p, _u64, _fp, _fp]),
    ('mi3d_stats_join'         , C.c_int   , [C.c_void_p, C.c_void_p]),
    ('mi3d_stats_chain'        , C.c_int   , [C.c_void_p, C.c_void_p]),
    ('mi3d_stats_end_run'      , C.c_int   , [C.c_void_p, _fp, _fp]),
    ('mi3d_stats_get'          , C.c_int   , [C.c_void_p, C.c_int, _fp, _fp, C.POINTER(C.c_int)]),
    ('mi3d_debug_philox'       , C.c_int   , [C.c_void_p, _u64, _u64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    ('mi3d_debug_order'        , C.c_int   , [C.c_void_p, _u64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int]),
    ('mi3d_debug_entry'        , C.c_int   , [C.c_void_p, _u64, _fp]),
    ('mi3d_debug_thermal'      , C.c_int   , [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), _u64]),
    ('mi3d_debug_backward'     , C.c_int   , [C.c_void_p, _u64, _u64, C.c_int, _fp, _dp, C.POINTER(_u64)]),
    ('mi3d_debug_backward_views', C.c_int  , [C.c_void_p, _u64, _u64, C.c_int, _fp, _fp, _dp, C.POINTER(_u64)]),
    ('mi3d_debug_phase_tables' , C.c_int   , [C.c_void_p, C.c_int, C.c_int, _fp, _fp, _fp, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]),
    ('mi3d_debug_phase'        , C.c_int   , [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp]),
    ('mi3d_debug_rotate'       , C.c_int   , [C.c_void_p, C.c_int, _fp, _fp, _fp, _fp, _fp]),
    ('mi3d_debug_surface'      , C.c_int   , [C.c_void_p, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp]),
]

TAB_IDX_N = 514     # entries of a bucket index into the phase tables (include/mi3d.h: MI3D_TAB_IDX_N)


def library_path():
    # MI3D_LIBRARY selects another build of the SAME library (kernel A/B experiments); never a fallback
    return os.environ.get('MI3D_LIBRARY') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libmi3drt.so')


def load_library():

    """
    Load libmi3drt.so (built in-tree by `__graft_entry__.build()` / `make -C er3t_amd/csrc`).
    Raises OSError when it is missing -- the product path never substitutes anything for it.
    """

    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            msg = 'Error [Mi3dSolver]: Cannot find <%s>. Build it with `python -c "import __graft_entry__ as g; g.build()"`.' % path
            raise OSError(msg)
        lib = C.CDLL(path)
        for name, restype, argtypes in _SIGNATURES:
            try:
                fn = getattr(lib, name)     # AttributeError here means the library is stale
            except AttributeError:
                if os.environ.get('MI3D_LIBRARY'):   # an older build in a kernel A/B experiment (tools/ab.py): what it lacks fails when called
                    setattr(lib, name, _stale(name, path))
                    continue
                msg = 'Error [Mi3dSolver]: <%s> is stale: it lacks <%s>. Rebuild it with `make -C er3t_amd/csrc`.' % (path, name)
                raise OSError(msg)
            fn.restype  = restype
            fn.argtypes = argtypes
        _LIB = lib
    return _LIB


def _stale(name, path):
    def missing(*args):
        msg = 'Error [Mi3dSolver]: library is stale: <%s> missing from <%s>.' % (name, path)
        raise OSError(msg)
    missing.stale = True
    return missing


def _ptr(a, typ=_fp):
    return None if a is None else a.ctypes.data_as(typ)


class Mi3dSolver:

    """
    One solver instance bound to one GPU.

        sol = Mi3dSolver(device=0)
        sol.load_scene(scene)                 # er3t_amd.scene.Scene
        sol.run(nphoton, seed=..., offset=0)  # asynchronous, accumulates
        rad  = sol.radiance(nphoton_total)    # (nview, nyr, nxr) float32
        flux = sol.flux(nphoton_total)        # (3, nz+1, ny, nx) float32
        heat = sol.heating(nphoton_total)     # (nz, ny, nx) float32, scene.target & TARGET_HEAT
    """

    def __init__(self, device=0):
        self.lib = load_library()
        self._h  = C.c_void_p()
        self._chk(self.lib.mi3d_create(int(device), C.byref(self._h)))
        self.device = device
        self.scene  = None

    def _chk(self, rc):
        if rc != 0:
            msg = 'Error [Mi3dSolver]: %s (code %d).' % (self.lib.mi3d_last_error().decode('utf-8', 'replace'), rc)
            raise OSError(msg)

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.mi3d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs ------------------------------------------------------------------------------
    def set_atm1d(self, zgrd, ext1d, omg1d, apf1d, abs1d):
        zgrd  = np.ascontiguousarray(zgrd, dtype=np.float64)
        ext1d = np.ascontiguousarray(np.atleast_2d(ext1d), dtype=np.float32)
        omg1d = np.ascontiguousarray(np.atleast_2d(omg1d), dtype=np.float32)
        apf1d = np.ascontiguousarray(np.atleast_2d(apf1d), dtype=np.float32)
        abs1d = np.ascontiguousarray(abs1d, dtype=np.float32)
        nz = zgrd.size - 1
        if ext1d.shape[1] != nz or omg1d.shape != ext1d.shape or apf1d.shape != ext1d.shape or abs1d.size != nz:
            raise ValueError('Error [Mi3dSolver]: 1-D profiles do not match <zgrd>.')
        self._chk(self.lib.mi3d_set_atm1d(self._h, nz, _ptr(zgrd, _dp), ext1d.shape[0], _ptr(ext1d), _ptr(omg1d), _ptr(apf1d), _ptr(abs1d)))

    def set_atm3d(self, nx, ny, dx, dy, nz3=0, iz3l=1, abst=None, extp=None, omgp=None, apfp=None):
        np3d = 0
        if nz3 > 0:
            extp = np.ascontiguousarray(extp, dtype=np.float32); omgp = np.ascontiguousarray(omgp, dtype=np.float32)
            apfp = np.ascontiguousarray(apfp, dtype=np.float32)
            if extp.ndim == 3:
                extp = extp[None]; omgp = omgp[None]; apfp = apfp[None]
            np3d = extp.shape[0]
            if extp.shape != (np3d, nz3, ny, nx) or omgp.shape != extp.shape or apfp.shape != extp.shape:
                raise ValueError('Error [Mi3dSolver]: 3-D arrays must be (np3d, nz3, ny, nx).')
            if abst is not None:
                abst = np.ascontiguousarray(abst, dtype=np.float32)
                if abst.shape != (nz3, ny, nx):
                    raise ValueError('Error [Mi3dSolver]: <abst> must be (nz3, ny, nx).')
        self._chk(self.lib.mi3d_set_atm3d(self._h, int(nx), int(ny), int(nz3), int(iz3l), int(np3d), float(dx), float(dy),
                                          _ptr(abst), _ptr(extp), _ptr(omgp), _ptr(apfp)))

    def set_phase(self, ang=None, pha=None):
        if pha is None:
            self._chk(self.lib.mi3d_set_phase(self._h, 0, 0, None, None))
            return
        ang = np.ascontiguousarray(ang, dtype=np.float32)
        pha = np.ascontiguousarray(np.atleast_2d(pha), dtype=np.float32)
        if pha.shape[1] != ang.size:
            raise ValueError('Error [Mi3dSolver]: <pha> must be (npf, nang).')
        self._chk(self.lib.mi3d_set_phase(self._h, ang.size, pha.shape[0], _ptr(ang), _ptr(pha)))

    def set_surface(self, mtype=1, param=(0.0, 0.0, 0.0, 0.0, 0.0)):
        p = np.zeros(5, dtype=np.float32)
        q = np.ravel(np.asarray(param, dtype=np.float32))
        p[:min(5, q.size)] = q[:5]
        self._chk(self.lib.mi3d_set_surface(self._h, int(mtype), _ptr(p)))

    def set_surface2d(self, jsfc, psfc):
        jsfc = np.ascontiguousarray(jsfc, dtype=np.float32)
        psfc = np.ascontiguousarray(psfc, dtype=np.float32)
        nyb, nxb = jsfc.shape
        if psfc.shape != (5, nyb, nxb):
            raise ValueError('Error [Mi3dSolver]: <psfc> must be (5, nyb, nxb).')
        self._chk(self.lib.mi3d_set_surface2d(self._h, nxb, nyb, None, _ptr(jsfc), _ptr(psfc)))

    def set_source(self, flx=1.0, qmax=0.533133, the=150.0, phi=270.0):
        self._chk(self.lib.mi3d_set_source(self._h, float(flx), float(qmax), float(the), float(phi)))

    def set_thermal(self, mtype=3, wlen=None, tmp1d=None, tmpa3d=None, tmps2d=None, fsol=None):
        """thermal source (Src_mtype = 3): band-centre wavelength <wlen> [um], (nz+1,) interface temperatures <tmp1d> [K], optional
        voxel anomalies <tmpa3d> (nz3, ny, nx) and surface anomalies <tmps2d> (nyb, nxb) [K]; mtype=1 switches back to the sun.
        mtype=2, solar+thermal: the same arguments plus <fsol>, the solar irradiance normal to the beam at the top of the atmosphere
        [W m-2 um-1] (include/mi3d.h: mi3d_set_solar_irradiance); the sun stands where set_source says"""
        if int(mtype) == 1:
            self._chk(self.lib.mi3d_set_thermal(self._h, 1, 0.0, 0, None, None, None))
            return
        tmp1d = np.ascontiguousarray(np.ravel(tmp1d), dtype=np.float32)
        if tmpa3d is not None:
            tmpa3d = np.ascontiguousarray(tmpa3d, dtype=np.float32)
        if tmps2d is not None:
            tmps2d = np.ascontiguousarray(tmps2d, dtype=np.float32)
        self._chk(self.lib.mi3d_set_thermal(self._h, int(mtype), float(wlen if wlen is not None else 0.0), tmp1d.size, _ptr(tmp1d),
                                            _ptr(tmpa3d), _ptr(tmps2d)))
        if fsol is not None:
            self._chk(self.lib.mi3d_set_solar_irradiance(self._h, float(fsol)))

    def source_power(self):
        """(P_tot, P_sol) [W um-1 per unit Src_flx] of a thermal or solar+thermal job: what its cells emit in all, and Src_fsol mu0 Lx Ly
        (0 for a thermal job); a photon is thermal with probability P_tot / (P_tot + P_sol).  Builds the source if needed, needs no run
        (include/mi3d.h: mi3d_get_source_power).  A solar job raises OSError"""
        ptot, psol = C.c_double(0.0), C.c_double(0.0)
        self._chk(self.lib.mi3d_get_source_power(self._h, C.byref(ptot), C.byref(psol)))
        return float(ptot.value), float(psol.value)

    def set_views(self, the, phi, zloc, zref=0.0, nxr=1, nyr=1):
        the = np.ascontiguousarray(np.atleast_1d(the), dtype=np.float64)
        phi = np.ascontiguousarray(np.atleast_1d(phi), dtype=np.float64)
        zloc = np.ascontiguousarray(np.atleast_1d(zloc), dtype=np.float64)
        if not (the.size == phi.size == zloc.size):
            raise ValueError('Error [Mi3dSolver]: view arrays differ in length.')
        self._chk(self.lib.mi3d_set_views(self._h, the.size, _ptr(the, _dp), _ptr(phi, _dp), _ptr(zloc, _dp), float(zref), int(nxr), int(nyr)))

    def set_cameras(self, the, phi, psi, xpos, ypos, zloc, qmax, umax, vmax, apsize, nxr, nyr):
        """all-sky cameras (Rad_mrkind = 1): point sensors at (xpos Lx, ypos Ly, zloc), Z-Y-Z rotations phi, the, psi"""
        arrs = [np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64) for a in (the, phi, psi, xpos, ypos, zloc, qmax, umax, vmax, apsize)]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise ValueError('Error [Mi3dSolver]: camera arrays differ in length.')
        self._chk(self.lib.mi3d_set_cameras(self._h, n, *[_ptr(a, _dp) for a in arrs], int(nxr), int(nyr)))

    def set_camera_map(self, mpmap=1, mrproj=0):
        """cameras' pixel map (Rad_mpmap: 1 polar, 2 rectangular) and weighting (Rad_mrproj: 0 mean radiance, 1 cosine-weighted)"""
        self._chk(self.lib.mi3d_set_camera_map(self._h, int(mpmap), int(mrproj)))

    def set_camera_method(self, method='forward'):
        """how the cameras and point radiometers of a thermal job are served (include/mi3d.h: mi3d_set_camera_method): 'forward' (0), the
        local estimates of forward photons, or 'backward' (1), histories that start at the sensor"""
        m = {'forward': 0, 'backward': 1}.get(method, method)
        if m not in (0, 1):
            raise ValueError('Error [Mi3dSolver]: <method=%r> must be \'forward\' (0) or \'backward\' (1).' % (method,))
        self._chk(self.lib.mi3d_set_camera_method(self._h, int(m)))

    def set_view_method(self, method='forward'):
        """how the satellite views of a thermal job are served (include/mi3d.h: mi3d_set_view_method): 'forward' (0), the local estimates of
        forward photons, or 'backward' (1), histories that start on the sensor plane of their pixel"""
        m = {'forward': 0, 'backward': 1}.get(method, method)
        if m not in (0, 1):
            raise ValueError('Error [Mi3dSolver]: <method=%r> must be \'forward\' (0) or \'backward\' (1).' % (method,))
        self._chk(self.lib.mi3d_set_view_method(self._h, int(m)))

    def set_emission_weights(self, on=True):
        """per-cell emission weights of the backward route (include/mi3d.h: mi3d_set_emission_weights): on, every run also tallies
        K[pixel][cell], the share of a pixel's reading that comes from a cell per unit Planck radiance there"""
        self._chk(self.lib.mi3d_set_emission_weights(self._h, 1 if on else 0))

    def set_view_profiles(self, on=True):
        """per-layer profiles of the backward route's satellite views (include/mi3d.h: mi3d_set_view_profiles): on, every run also tallies
        the weighting function K[pixel][layer | surface] and the contribution C[pixel][layer | surface] of every pixel.  True / False or
        the value itself (anything but 0 and 1 is refused by the library)"""
        self._chk(self.lib.mi3d_set_view_profiles(self._h, int(on)))

    def set_pixel_errors(self, on=True):
        """per-pixel standard errors of the backward routes (include/mi3d.h: mi3d_set_pixel_errors): on, every run also tallies the squared
        score of every history in its pixel, and radiance_se() reads the standard error of every pixel's mean.  True / False or the value
        itself (anything but 0 and 1 is refused by the library)"""
        self._chk(self.lib.mi3d_set_pixel_errors(self._h, int(on)))

    def set_view_sunlight(self, on=True):
        """the sunlight term of the backward route's satellite views (include/mi3d.h: mi3d_set_view_sunlight): on, the route serves a
        solar+thermal job (Src_mtype = 2): every scattering and every surface reflection of a history also scores the sunlight it turns into
        the line of sight.  True / False or the value itself (anything but 0 and 1 is refused by the library)"""
        self._chk(self.lib.mi3d_set_view_sunlight(self._h, int(on)))

    def set_view_columns(self, on=True):
        """the backward route's satellite views under independent columns and partial 3-D (include/mi3d.h: mi3d_set_view_columns): on, the
        route serves solver 2 (IPA) and 1 (partial 3-D) -- a history keeps the column under its start and crosses every layer level to level.
        True / False or the value itself (anything but 0 and 1 is refused by the library)"""
        self._chk(self.lib.mi3d_set_view_columns(self._h, int(on)))

    def set_options(self, target=TARGET_FLUX, solver=0, wmin=0.2, wfac=1.0, column_le=True):
        self._chk(self.lib.mi3d_set_options(self._h, int(target), int(solver), float(wmin), float(wfac), 1 if column_le else 0))

    def set_le_roulette(self, tau1=0.0):
        self._chk(self.lib.mi3d_set_le_roulette(self._h, float(tau1)))

    def set_le_weight_roulette(self, cmin=0.0):
        self._chk(self.lib.mi3d_set_le_weight_roulette(self._h, float(cmin)))

    def set_heating_estimator(self, estimator=0):
        """the heating-rate tally's estimator (include/mi3d.h: mi3d_set_heating_estimator): 0 collision, 1 path length"""
        self._chk(self.lib.mi3d_set_heating_estimator(self._h, int(estimator)))

    def set_counting(self, on=True):
        self._chk(self.lib.mi3d_set_counting(self._h, 1 if on else 0))

    def load_scene(self, scene, column_le=True):
        s = scene
        self.set_atm1d(s.zgrd, s.ext1d, s.omg1d, s.apf1d, s.abs1d)
        self.set_atm3d(s.nx, s.ny, s.dx, s.dy, nz3=s.nz3, iz3l=s.iz3l, abst=s.abst, extp=s.extp, omgp=s.omgp, apfp=s.apfp)
        self.set_phase(s.ang, s.pha)
        if s.jsfc is not None:
            self.set_surface2d(s.jsfc, s.psfc)
        else:
            self.set_surface(s.sfc_mtype, s.sfc_param)
        self.set_source(s.src_flx, s.src_qmax, s.src_the, s.src_phi)
        if getattr(s, 'src_mtype', 1) in (2, 3):
            self.set_thermal(s.src_mtype, s.src_wlen, s.tmp1d, s.tmpa3d, s.tmps2d, fsol=s.src_fsol if s.src_mtype == 2 else None)
        else:
            self.set_thermal(1)
        if getattr(s, 'rad_kind', 2) == 1 and s.nview > 0:
            self.set_cameras(s.view_the, s.view_phi, s.cam_psi, s.cam_xpos, s.cam_ypos, s.view_zloc, s.cam_qmax, s.cam_umax, s.cam_vmax,
                             s.cam_apsize, s.nxr, s.nyr)
            self.set_camera_map(getattr(s, 'cam_mpmap', 1), getattr(s, 'cam_mrproj', 0))
            self.set_tuning(cam_images=int(getattr(s, 'cam_images', -1)))
        else:
            self.set_views(s.view_the, s.view_phi, s.view_zloc, zref=s.zref, nxr=s.nxr, nyr=s.nyr)
        self.set_camera_method(int(getattr(s, 'cam_method', 0)))
        self.set_view_method(int(getattr(s, 'view_method', 0)))
        self.set_emission_weights(int(getattr(s, 'cam_weights', 0)))
        # (an older build in a kernel A/B experiment, MI3D_LIBRARY, has no such switch: it is off there, and asking for it fails)
        if int(getattr(s, 'view_profiles', 0)) or not getattr(self.lib.mi3d_set_view_profiles, 'stale', False):
            self.set_view_profiles(int(getattr(s, 'view_profiles', 0)))
        if int(getattr(s, 'pixel_errors', 0)) or not getattr(self.lib.mi3d_set_pixel_errors, 'stale', False):      # (likewise)
            self.set_pixel_errors(int(getattr(s, 'pixel_errors', 0)))
        if int(getattr(s, 'view_sunlight', 0)) or not getattr(self.lib.mi3d_set_view_sunlight, 'stale', False):    # (likewise)
            self.set_view_sunlight(int(getattr(s, 'view_sunlight', 0)))
        if int(getattr(s, 'view_columns', 0)) or not getattr(self.lib.mi3d_set_view_columns, 'stale', False):      # (likewise)
            self.set_view_columns(int(getattr(s, 'view_columns', 0)))
        self.set_options(s.target, s.solver, s.wmin, s.wfac, column_le)
        self.set_heating_estimator(int(getattr(s, 'heat_estimator', 0)))
        self.set_le_roulette(getattr(s, 'le_tau1', 0.0))
        self.set_le_weight_roulette(getattr(s, 'le_cmin', 0.0))
        self.scene = s
        self._shape_rad  = (s.nview, s.nyr, s.nxr)
        self._shape_flux = (3, s.nz+1, s.ny, s.nx)
        self.prepare()

    def update_atm1d(self, scene):
        """swap the 1-D profiles only (the per-g part of a correlated-k loop); 3-D arrays stay on the device"""
        self.set_atm1d(scene.zgrd, scene.ext1d, scene.omg1d, scene.apf1d, scene.abs1d)
        self.prepare()

    # ---- execution ---------------------------------------------------------------------------
    def bind(self, rad_ptr=None, flux_ptr=None, stream=None, heat_ptr=None, wgt_ptr=None, prf_ptr=None, err_ptr=None):
        self._chk(self.lib.mi3d_bind_device_buffers(self._h, C.c_void_p(rad_ptr or 0), C.c_void_p(flux_ptr or 0), C.c_void_p(stream or 0)))
        self._chk(self.lib.mi3d_bind_heating_buffer(self._h, C.c_void_p(heat_ptr or 0)))
        self._chk(self.lib.mi3d_bind_weights_buffer(self._h, C.c_void_p(wgt_ptr or 0)))
        if prf_ptr or not getattr(self.lib.mi3d_bind_view_profiles_buffer, 'stale', False):      # (likewise, load_scene)
            self._chk(self.lib.mi3d_bind_view_profiles_buffer(self._h, C.c_void_p(prf_ptr or 0)))
        if err_ptr or not getattr(self.lib.mi3d_bind_pixel_errors_buffer, 'stale', False):       # (likewise)
            self._chk(self.lib.mi3d_bind_pixel_errors_buffer(self._h, C.c_void_p(err_ptr or 0)))

    def prepare(self):
        self._chk(self.lib.mi3d_prepare(self._h))

    def reset(self):
        self._chk(self.lib.mi3d_reset(self._h))

    def run(self, nphoton, seed=1, offset=0):
        self._chk(self.lib.mi3d_run(self._h, int(nphoton), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset)))

    def sync(self):
        self._chk(self.lib.mi3d_sync(self._h))

    def set_kernel(self, general=False):
        """general=True: always the general kernel build (k_transport), also where the lean ones apply (A/B and parity tests)"""
        self._chk(self.lib.mi3d_set_kernel(self._h, 1 if general else 0))

    def set_tuning(self, **knobs):
        """launch-machinery knobs (include/mi3d.h: mi3d_set_tuning), e.g. set_tuning(evcap_log2=12, own_stream=1);
        keys: tile_cols, batch_log2, evcap_log2, rad_spread, own_stream, tally_lists, tlcap_log2, entry_records (0 none, 1 short where allowed, 2 long always), cam_images,
        tally_window, rad_row_pad, vpad_col, vpad_row, overlap_rays, overlap_sort, overlap_pre, tl_split, rays_wg, emit_wg, wgt_stage"""
        for key, value in knobs.items():
            self._chk(self.lib.mi3d_set_tuning(self._h, key.encode(), int(value)))

    def kernel_name(self):
        """which build of the transport kernel served the last run (for logs; results do not depend on it)"""
        return self.lib.mi3d_last_kernel(self._h).decode()

    def timing(self):
        ms = C.c_double(0.0); n = _u64(0)
        self._chk(self.lib.mi3d_get_timing(self._h, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    # ---- results -----------------------------------------------------------------------------
    def radiance(self, nphoton_total):
        out = np.zeros(self._shape_rad, dtype=np.float32)
        if out.size:
            self._chk(self.lib.mi3d_get_radiance(self._h, int(nphoton_total), _ptr(out)))
        return out

    def radiance_se(self, nphoton_total):
        """the standard error of every pixel of radiance(nphoton_total), float32 (nview, nyr, nxr), from the histories of the runs since the
        last reset (include/mi3d.h: mi3d_get_radiance_se); needs set_pixel_errors(1) and a run on a backward route"""
        out = np.zeros(self._shape_rad, dtype=np.float32)
        self._chk(self.lib.mi3d_get_radiance_se(self._h, int(nphoton_total), _ptr(out)))
        return out

    def run_until(self, se_max, relative=False, max_histories=1 << 30, seed=1, chunk=None):
        """run the job loaded, from a reset, until its image is as quiet as asked: chunks of histories at offsets that continue the id range
        [0, N) -- the normalisation rule of radiance() --, every chunk a multiple of the number of pixels, until the largest standard error
        of a pixel (radiance_se) is at most <se_max>, or <se_max> times the pixel's radiance with relative=True, or until the next chunk
        would pass <max_histories>.  Returns N: radiance(N) and radiance_se(N) are the results, those of one run(N, seed).  <chunk>: the
        histories of a chunk (rounded up to a multiple of the pixels; default 1024 a pixel).  Single process; needs set_pixel_errors(1)"""
        s = self.scene
        npix = s.nview*s.nyr*s.nxr
        if npix < 1 or not (se_max >= 0.0):
            raise ValueError('Error [Mi3dSolver]: run_until needs an image and <se_max> >= 0.')
        per = max(1, -(-int(chunk)//npix)) if chunk else 1024
        nmax = (int(max_histories)//npix)*npix
        if nmax < npix:
            raise ValueError('Error [Mi3dSolver]: <max_histories=%d> is less than one history a pixel (%d pixels).' % (max_histories, npix))
        self.reset()
        n = 0
        while n < nmax:
            nb = min(per*npix, nmax-n)
            self.run(nb, seed=seed, offset=n)
            n += nb
            se = self.radiance_se(n)
            if n < 2*npix:
                continue                       # (a pixel with one history reads 0: no error is known yet)
            if relative:
                if np.all(se <= se_max*np.abs(self.radiance(n))):
                    break
            elif float(se.max()) <= se_max:
                break
        return n

    def weights_shape(self):
        """(npix, nvox, nz, nsfc) of the emission weights' tally for the scene loaded: K_raw is [npix][nvox + nz + nsfc] float64"""
        s = self.scene
        nsfc = int(s.jsfc.size) if s.jsfc is not None else 1
        return s.nview*s.nyr*s.nxr, s.nx*s.ny*s.nz3, s.nz, nsfc

    def emission_weights(self, nphoton_total):
        """the per-cell emission weights of the backward route (include/mi3d.h: mi3d_get_emission_weights) for a job of nphoton_total ids:
        'voxels' (npix, nz3, ny, nx), 'layers' (npix, nz), 'surface' (npix, nyb, nxb) -- 1 x 1 for a uniform surface -- and 'planck',
        the float32 Planck radiances the kernel multiplied with, in the same three shapes without npix.  The reading of pixel p is
        Src_flx sum_c K[p][c] planck[c] over all three parts"""
        s = self.scene
        npix, nvox, nz, nsfc = self.weights_shape()
        ncell = nvox+nz+nsfc
        k = np.zeros((npix, ncell), dtype=np.float32)
        b = np.zeros(ncell, dtype=np.float32)
        self._chk(self.lib.mi3d_get_emission_weights(self._h, int(nphoton_total), _ptr(k), _ptr(b)))
        sshape = s.jsfc.shape if s.jsfc is not None else (1, 1)
        return {'voxels': k[:, :nvox].reshape(npix, s.nz3, s.ny, s.nx), 'layers': k[:, nvox:nvox+nz], 'surface': k[:, nvox+nz:].reshape((npix,)+tuple(sshape)),
                'planck': {'voxels': b[:nvox].reshape(s.nz3, s.ny, s.nx), 'layers': b[nvox:nvox+nz], 'surface': b[nvox+nz:].reshape(sshape)}}

    def view_profiles(self, nphoton_total):
        """the per-layer profiles of the backward route's satellite views (include/mi3d.h: mi3d_get_view_profiles) for a job of
        nphoton_total ids: 'weight' and 'contribution', float32 (nview, nyr, nxr, nz + 1) -- rows 0 ... nz - 1 the layers from the surface
        up, row nz the surface.  The radiance of pixel p is Src_flx contribution[p].sum()"""
        s = self.scene
        shape = (s.nview, s.nyr, s.nxr, s.nz+1)
        k = np.zeros(shape, dtype=np.float32)
        c = np.zeros(shape, dtype=np.float32)
        self._chk(self.lib.mi3d_get_view_profiles(self._h, int(nphoton_total), _ptr(k), _ptr(c)))
        return {'weight': k, 'contribution': c}

    def flux(self, nphoton_total):
        out = np.zeros(self._shape_flux, dtype=np.float32)
        self._chk(self.lib.mi3d_get_flux(self._h, int(nphoton_total), _ptr(out)))
        return out

    def direct_levels(self):
        """(nz+1,) the known part of the direct beam that mi3d_get_flux adds to the tallies, for the job that ran last"""
        out = np.zeros(self.scene.nz+1, dtype=np.float64)
        self._chk(self.lib.mi3d_get_direct_levels(self._h, _ptr(out, _dp)))
        return out

    def camera_direct(self):
        """(nview, nyr, nxr) float64: the direct sun in the cameras (include/mi3d.h: mi3d_get_camera_direct), units of radiance();
        known, not tallied, and not part of radiance()"""
        out = np.zeros(self._shape_rad, dtype=np.float64)
        if out.size:
            self._chk(self.lib.mi3d_get_camera_direct(self._h, _ptr(out, _dp)))
        return out

    def heating(self, nphoton_total):
        """absorbed power per unit volume and unit Src_flx, (nz, ny, nx): jobs whose target includes TARGET_HEAT (Flx_mhrt = 1).
        Thermal job (Flx_mhrt = 2): the NET, absorbed - emitted [W m-3 um-1 per unit Src_flx], negative where the cell cools; the
        emitted part is emission(), known and not tallied.  The surface is not part of the grid: its net gain is fdn - fup at level 0
        of flux()"""
        s = self.scene
        out = np.zeros((s.nz, s.ny, s.nx), dtype=np.float32)
        self._chk(self.lib.mi3d_get_heating(self._h, int(nphoton_total), _ptr(out)))
        return out

    def emission(self):
        """(nz, ny, nx) float32: what every cell of a thermal job emits per unit volume, Src_flx 4 pi ka B(T), in the units of heating()
        (include/mi3d.h: mi3d_get_emission); absorbed = heating() + emission().  A solar job raises OSError"""
        s = self.scene
        out = np.zeros((s.nz, s.ny, s.nx), dtype=np.float32)
        self._chk(self.lib.mi3d_get_emission(self._h, _ptr(out)))
        return out

    # ---- run statistics on the device (sum over g per run, mean / std over runs) ---------------
    def stats_begin(self, rad_run_ptr=None, flux_run_ptr=None):
        self._chk(self.lib.mi3d_stats_begin(self._h, C.c_void_p(rad_run_ptr or 0), C.c_void_p(flux_run_ptr or 0)))

    def stats_join(self, owner):
        """this handle adds its jobs into the run fields of <owner> (another Mi3dSolver on the same device that has begun statistics)"""
        self._chk(self.lib.mi3d_stats_join(self._h, owner._h))

    def stats_chain(self, after):
        """this handle's next statistics kernel waits for the last one of <after> (another Mi3dSolver on the same device)"""
        self._chk(self.lib.mi3d_stats_chain(self._h, after._h))

    def stats_set_analytic_share(self, share):
        """photon-sharded jobs: 1 on the rank that adds the analytic direct beam to the run field, 0 on the others"""
        self._chk(self.lib.mi3d_stats_set_analytic_share(self._h, float(share)))

    def stats_add(self, nphoton_total, factor_rad=None, factor_flux=None):
        s = self.scene
        fr = ff = None
        if factor_rad is not None:
            fr = np.ascontiguousarray(np.broadcast_to(np.asarray(factor_rad, dtype=np.float32), (s.nview,)))
        if factor_flux is not None:
            ff = np.ascontiguousarray(np.broadcast_to(np.asarray(factor_flux, dtype=np.float32), (s.nz+1,)))
        self._chk(self.lib.mi3d_stats_add(self._h, int(nphoton_total), _ptr(fr), _ptr(ff)))

    def stats_end_run(self, keep=False):
        """close the run; with keep=True also return its fields {'rad': ..., 'flux': ...} (host copies)"""
        s = self.scene
        rad = np.zeros(self._shape_rad, dtype=np.float32) if keep and (s.target & TARGET_RADIANCE) else None
        flux = np.zeros(self._shape_flux, dtype=np.float32) if keep and (s.target & TARGET_FLUX) else None
        self._chk(self.lib.mi3d_stats_end_run(self._h, _ptr(rad), _ptr(flux)))
        out = {}
        if rad is not None:
            out['rad'] = rad
        if flux is not None:
            out['flux'] = flux
        return out

    def stats_get(self, which):
        """(mean, std, nrun) over the closed runs; which = TARGET_RADIANCE or TARGET_FLUX"""
        shape = self._shape_rad if which == TARGET_RADIANCE else self._shape_flux
        mean = np.zeros(shape, dtype=np.float32); sdev = np.zeros(shape, dtype=np.float32); n = C.c_int(0)
        self._chk(self.lib.mi3d_stats_get(self._h, int(which), _ptr(mean), _ptr(sdev), C.byref(n)))
        return mean, sdev, int(n.value)

    def counters(self):
        out = np.zeros(NCOUNTER, dtype=np.uint64)
        self._chk(self.lib.mi3d_get_counters(self._h, out.ctypes.data_as(C.POINTER(_u64))))
        return dict(zip(COUNTER_NAMES, (int(v) for v in out)))

    def debug_order(self, n, ntile_max=1024):
        """test hook: (photon order of the last launch: n indices sorted by start tile, where each tile's piece ends)"""
        order = np.zeros(n, dtype=np.uint32); tend = np.zeros(ntile_max, dtype=np.uint32)
        self._chk(self.lib.mi3d_debug_order(self._h, int(n), order.ctypes.data_as(C.POINTER(C.c_uint32)), tend.ctypes.data_as(C.POINTER(C.c_uint32)), int(ntile_max)))
        return order, tend

    def debug_entry(self, n=0):
        """test hook: (form, records) of the last launch of the last run: form 3 the long entry records (48 bytes a photon), 2 the short
        ones (32 bytes); records: the first n as they lie in memory, float32 [ceil(n / 64), form, 64, 4] (blocks of 64 photons, part by
        part), or None for n = 0.  A launch without entry records raises OSError (include/mi3d.h: mi3d_debug_entry)"""
        form = self.lib.mi3d_debug_entry(self._h, 0, None)
        if form < 0:
            self._chk(form)
        if not n:
            return form, None
        rec = np.zeros(((int(n) + 63)//64, form, 64, 4), dtype=np.float32)
        rc = self.lib.mi3d_debug_entry(self._h, int(n), _ptr(rec))
        if rc < 0:
            self._chk(rc)
        return form, rec

    def debug_thermal(self, ncell):
        """test hook: (P_tot, the device CDF [ncell] float64) of the thermal source the last mi3d_prepare built"""
        ptot = C.c_double(0.0); cdf = np.zeros(int(ncell), dtype=np.float64)
        self._chk(self.lib.mi3d_debug_thermal(self._h, C.byref(ptot), cdf.ctypes.data_as(C.POINTER(C.c_double)), int(ncell)))
        return float(ptot.value), cdf

    def debug_backward(self, seed, id0, n):
        """test hook of the backward route: (directions (n, 3) float32 away from the sensor, scores (n,) float64 as they enter the raw
        tally, capped histories of the runs since the last reset) for the ids id0 .. id0 + n - 1 (include/mi3d.h: mi3d_debug_backward)"""
        d = np.zeros((int(n), 3), dtype=np.float32); sc = np.zeros(int(n), dtype=np.float64); cap = _u64(0)
        self._chk(self.lib.mi3d_debug_backward(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(id0), int(n), _ptr(d), _ptr(sc, _dp), C.byref(cap)))
        return d, sc, int(cap.value)

    def debug_backward_views(self, seed, id0, n):
        """test hook of the backward route for satellite views: (start points (n, 3) float32, directions (n, 3) float32 of flight, scores
        (n,) float64 as they enter the raw tally, capped histories of the runs since the last reset) for the ids id0 .. id0 + n - 1
        (include/mi3d.h: mi3d_debug_backward_views)"""
        st = np.zeros((int(n), 3), dtype=np.float32); d = np.zeros((int(n), 3), dtype=np.float32); sc = np.zeros(int(n), dtype=np.float64); cap = _u64(0)
        self._chk(self.lib.mi3d_debug_backward_views(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(id0), int(n), _ptr(st), _ptr(d), _ptr(sc, _dp),
                                                     C.byref(cap)))
        return st, d, sc, int(cap.value)

    def debug_phase_tables(self, nang, npf):
        """test hook: the device's phase tables after set_phase + prepare: (mu [nang], p [npf, nang], cdf [npf, nang]) float32 and the
        bucket indices (mu_idx [TAB_IDX_N], cdf_idx [npf, TAB_IDX_N]) uint16"""
        mu = np.zeros(nang, dtype=np.float32); p = np.zeros((npf, nang), dtype=np.float32); cdf = np.zeros((npf, nang), dtype=np.float32)
        mi = np.zeros(TAB_IDX_N, dtype=np.uint16); ci = np.zeros((npf, TAB_IDX_N), dtype=np.uint16)
        u16 = C.POINTER(C.c_uint16)
        self._chk(self.lib.mi3d_debug_phase_tables(self._h, int(nang), int(npf), _ptr(mu), _ptr(p), _ptr(cdf), _ptr(mi, u16), _ptr(ci, u16)))
        return mu, p, cdf, mi, ci

    def debug_phase(self, path, apf, x, usel=None, tab_lo=0, tab_n=0):
        """test hook: (P(apf, mu = x), mu(apf, u = x, usel)) float32 per point from the device's own routines; path 0: phase_eval /
        phase_sample on the tables in global memory, 1: through an LDS copy of tables tab_lo .. tab_lo + tab_n - 1, 2: the lean kernels'
        lean_phase_eval / lean_phase_sample on the staged tables, 3: the analytic copies (include/mi3d.h: mi3d_debug_phase)"""
        x = np.ascontiguousarray(np.ravel(x), dtype=np.float32)
        apf = np.ascontiguousarray(np.broadcast_to(np.asarray(apf, dtype=np.float32), x.shape))
        usel = np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if usel is None else usel, dtype=np.float32), x.shape))
        p = np.zeros(x.size, dtype=np.float32); m = np.zeros(x.size, dtype=np.float32)
        self._chk(self.lib.mi3d_debug_phase(self._h, int(path), int(tab_lo), int(tab_n), x.size, _ptr(apf), _ptr(x), _ptr(usel), _ptr(p), _ptr(m)))
        return p, m

    def debug_rotate(self, dirs, mu, uphi):
        """test hook: (directions (n, 3) float32 after rotate_dir(dirs[i], mu[i], uphi[i]), (n, 2) float32 sine and cosine of sincos_turns(uphi[i]))
        from the device's own routines (include/mi3d.h: mi3d_debug_rotate)"""
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        mu = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float32), d.shape[:1]))
        uphi = np.ascontiguousarray(np.broadcast_to(np.asarray(uphi, dtype=np.float32), d.shape[:1]))
        out = np.zeros_like(d); sc = np.zeros((d.shape[0], 2), dtype=np.float32)
        self._chk(self.lib.mi3d_debug_rotate(self._h, d.shape[0], _ptr(d), _ptr(mu), _ptr(uphi), _ptr(out), _ptr(sc)))
        return out, sc

    def debug_surface(self, path, sfc_type, param, din, dout=None):
        """test hook: float32 per point from the device's own surface routines; path 0: surface_R(Sfc{sfc_type, param[0..4]}, din[i], dout[i]),
        1: fresnel_unpolarised(param[2], param[3], din[i]), 2: dsm_shadow_lambda(din[i], param[0]); din: (n, 3) for path 0, (n,) for paths
        1 and 2 (include/mi3d.h: mi3d_debug_surface)"""
        par = np.zeros(5, dtype=np.float32)
        par[:len(param)] = np.asarray(param, dtype=np.float32)
        if int(path) == 0:
            a = np.ascontiguousarray(din, dtype=np.float32).reshape(-1, 3)
            b = np.ascontiguousarray(dout, dtype=np.float32).reshape(-1, 3)
            if a.shape != b.shape:
                raise ValueError('debug_surface: din and dout differ in shape')
        else:
            x = np.ascontiguousarray(np.ravel(din), dtype=np.float32)
            a = np.zeros((x.size, 3), dtype=np.float32); a[:, 0] = x
            b = None
        out = np.zeros(a.shape[0], dtype=np.float32)
        self._chk(self.lib.mi3d_debug_surface(self._h, int(path), a.shape[0], int(sfc_type), _ptr(par), _ptr(a), None if b is None else _ptr(b), _ptr(out)))
        return out

    def philox(self, seed, id0, draw, n):
        out = np.zeros((n, 4), dtype=np.uint32)
        self._chk(self.lib.mi3d_debug_philox(self._h, int(seed), int(id0), int(draw), int(n), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out
