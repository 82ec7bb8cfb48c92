"""
Scene: the solver's complete input for one (run, g) job, as plain arrays.

It is the in-memory equivalent of one MCARaTS input namelist plus its three side files
(reference: er3t/rtm/mca/mca_inp.py:15-384 for the keys, er3t/rtm/mca/mca_atm.py:373-389,
mca_sca.py:82-92 and mca_sfc.py:136-146 for the files).  All multi-dimensional arrays are C-order
numpy arrays whose LAST index is x, i.e. they have exactly the byte image of the reference's
"x fastest, then y, then z" Fortran-order files.

`from_nml` builds a Scene from a namelist dictionary of the shape `mcarats_ng` assembles
(er3t/rtm/mca/mcarats.py:234-414) and the directory holding the side files.
"""

import os
import re
from dataclasses import dataclass, field

import numpy as np

__all__ = ['Scene', 'TARGET_FLUX', 'TARGET_RADIANCE', 'TARGET_HEAT', 'SOLVER_3D', 'SOLVER_P3D', 'SOLVER_IPA']

TARGET_FLUX     = 1
TARGET_RADIANCE = 2
TARGET_HEAT     = 4     # heating rates beside the fluxes (Flx_mhrt = 1, er3t/rtm/mca/mcarats.py:279-283): with TARGET_FLUX
                        # (thermal job, Flx_mhrt = 2, a value of this project: the NET heating rate, absorbed - emitted)

SOLVER_3D  = 0
SOLVER_P3D = 1
SOLVER_IPA = 2


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@dataclass
class Scene:

    # 1-D background (Atm_zgrd0, Atm_ext1d(1:,ip), Atm_omg1d, Atm_apf1d, Atm_abs1d)
    zgrd : np.ndarray                     # (nz+1,) float64 [m]
    ext1d: np.ndarray                     # (np1d, nz) float32 [1/m]
    omg1d: np.ndarray                     # (np1d, nz)
    apf1d: np.ndarray                     # (np1d, nz)
    abs1d: np.ndarray                     # (nz,)

    # horizontal grid (Atm_nx, Atm_ny, Atm_dx, Atm_dy)
    nx: int = 1
    ny: int = 1
    dx: float = 1.0e4
    dy: float = 1.0e4

    # 3-D region (Atm_nz3, Atm_iz3l, Atm_np3d, Atm_inpfile)
    nz3 : int = 0
    iz3l: int = 1
    abst: np.ndarray = None               # (nz3, ny, nx) or None
    extp: np.ndarray = None               # (np3d, nz3, ny, nx)
    omgp: np.ndarray = None
    apfp: np.ndarray = None

    # tabulated phase functions (Sca_npf, Sca_nangi, Sca_inpfile)
    ang: np.ndarray = None                # (nang,) degrees
    pha: np.ndarray = None                # (npf, nang)

    # surface: uniform (Sfc_mtype, Sfc_param) or 2-D (Sfc_nxb, Sfc_nyb, Sfc_inpfile)
    sfc_mtype: int = 1
    sfc_param: np.ndarray = field(default_factory=lambda: np.array([0.0, 0, 0, 0, 0], dtype=np.float32))
    jsfc: np.ndarray = None               # (nyb, nxb) float32
    psfc: np.ndarray = None               # (5, nyb, nxb) float32

    # source (Src_flx, Src_qmax, Src_the, Src_phi)
    src_flx : float = 1.0
    src_qmax: float = 0.533133
    src_the : float = 150.0
    src_phi : float = 270.0
    # thermal source (Src_mtype = 3, include/mi3d.h: mi3d_set_thermal): band-centre wavelength Src_wlen [um], the nz+1 interface
    # temperatures Atm_tmp1d [K], voxel anomalies Atm_tmpa3d (nz3, ny, nx) and surface anomalies Sfc_tmps2d (nyb, nxb) [K] or None
    src_mtype: int = 1
    src_wlen : float = None
    tmp1d : np.ndarray = None
    tmpa3d: np.ndarray = None
    tmps2d: np.ndarray = None
    # solar+thermal source (Src_mtype = 2): the inputs of the thermal source plus Src_fsol (a key of this project), the solar spectral
    # irradiance on a plane normal to the beam at the top of the atmosphere [W m-2 um-1]; the sun stands where src_the, src_phi say
    src_fsol : float = None

    # radiance views (Rad_the, Rad_phi, Rad_zloc, Rad_zref, Rad_nxr, Rad_nyr)
    view_the : list = field(default_factory=list)
    view_phi : list = field(default_factory=list)
    view_zloc: list = field(default_factory=list)
    zref: float = 0.0
    nxr : int = 1
    nyr : int = 1
    # Rad_mrkind: 2 radiance averaged over the pixel's column cross-section (satellite); 1 local radiance at a point averaged
    # over the pixel's solid angle (all-sky camera, er3t/rtm/mca/mcarats.py:291-296): view i is then a camera at
    # (cam_xpos Lx, cam_ypos Ly, view_zloc) turned by the Z-Y-Z rotations view_phi, view_the, cam_psi, cone of view cam_qmax,
    # image cam_umax x cam_vmax degrees wide in the polar map (Rad_xpos, Rad_ypos, Rad_psi, Rad_qmax, Rad_umax, Rad_vmax),
    # nearest distance counted cam_apsize metres (Rad_apsize)
    rad_kind : int = 2
    cam_xpos : list = field(default_factory=list)
    cam_ypos : list = field(default_factory=list)
    cam_psi  : list = field(default_factory=list)
    cam_qmax : list = field(default_factory=list)
    cam_umax : list = field(default_factory=list)
    cam_vmax : list = field(default_factory=list)
    cam_apsize: list = field(default_factory=list)
    # cameras' pixel map and weighting (Rad_mpmap, Rad_mrproj; include/mi3d.h: mi3d_set_camera_map): 1 polar / 2 rectangular
    # (U = theta in [0, umax], V = phi in [-vmax, vmax]); 0 mean radiance / 1 cosine-weighted.  One pixel over the hemisphere with
    # the rectangular map is a point irradiance (mrproj 1) or actinic-flux (mrproj 0) sensor (er3t/rtm/mca/mca_inp.py:306-311)
    cam_mpmap : int = 1
    cam_mrproj: int = 0
    cam_images: int = -1                  # (-1: 2 where the ray kernel serves the job -- the default route --, else the nearest image alone, with a warning) the domain is cyclic: an event contributes to the periodic images of a camera within this many
                                          # domain lengths of the nearest one, the farther ones by Russian roulette on (r0 / r)^2 (unbiased).  er3t's
                                          # camera looks 89 degrees off its axis (mcarats.py:291-296); on the 12.8 km bench grid the nearest image
                                          # alone is complete to 75 degrees, lacks 43 % of the light at 82-86 and 96 % at 86-89; 1 / 2 / 3 images
                                          # recover 79 / 98 / 100 % of the last ring at 0.49 / 0.29 / 0.19 of the speed (profiles/r04/camera_images.log)

    cam_method: int = 0                   # Rad_mbwd (a key of this project; include/mi3d.h: mi3d_set_camera_method): 0 the forward route, 1 backward
                                          # Monte Carlo -- thermal cameras and point radiometers only; cam_images is then not used
    view_method: int = 0                  # Rad_mvbwd (a key of this project; include/mi3d.h: mi3d_set_view_method): 0 the forward route, 1 backward
                                          # Monte Carlo for the satellite views (rad_kind = 2) of a thermal job
    cam_weights: int = 0                  # Rad_mwgt (a key of this project; include/mi3d.h: mi3d_set_emission_weights): 1 the backward route also
                                          # tallies the per-cell emission weights K[pixel][cell] of every sensor; needs cam_method = 1
    view_profiles: int = 0                # Rad_mvprf (a key of this project; include/mi3d.h: mi3d_set_view_profiles): 1 the backward route also
                                          # tallies every pixel's weighting function and contribution per layer and for the surface;
                                          # needs rad_kind = 2, view_method = 1
    pixel_errors: int = 0                 # Rad_mserr (a key of this project; include/mi3d.h: mi3d_set_pixel_errors): 1 the backward route also
                                          # tallies the squared scores of every pixel, for its standard error from one run; needs
                                          # cam_method = 1 or view_method = 1, without cam_weights and view_profiles
    view_sunlight: int = 0                # Rad_mvsun (a key of this project; include/mi3d.h: mi3d_set_view_sunlight): 1 the backward route for
                                          # satellite views serves a solar+thermal job (src_mtype = 2): every scattering and reflection
                                          # also scores its sunlight; needs rad_kind = 2, view_method = 1, without view_profiles
    view_columns: int = 0                 # Rad_mvcol (a key of this project; include/mi3d.h: mi3d_set_view_columns): 1 the backward route for
                                          # satellite views serves independent columns and partial 3-D (solver = 2 / 1): a history keeps
                                          # its column; needs rad_kind = 2, view_method = 1, not under the 3-D solver

    # job
    target: int = TARGET_FLUX
    solver: int = SOLVER_3D
    wmin  : float = 0.2                   # Pho_wmin: Russian roulette below this weight ...
    wfac  : float = 1.0                   # Pho_wfac: ... survivors continue with this weight
    heat_estimator: int = 0               # Flx_mhest (a key of this project; include/mi3d.h: mi3d_set_heating_estimator): the heating-rate
                                          # tally's estimator, 0 collision, 1 path length (w kappa_a l per flight segment and cell)
    le_tau1: float = 2.0                  # Russian roulette on marched local-estimate rays beyond this optical depth (unbiased;
                                          # +64 % results per second on the nine-view configuration at 0.5 % more noise per photon); 0 = off

    le_cmin: float = 0.0796               # Russian roulette on the weight of marched local-estimate rays below this value, 1/(4 pi): the
                                          # estimates that look where the phase function is below its isotropic value (unbiased;
                                          # include/mi3d.h: mi3d_set_le_weight_roulette; nine-view configuration: 1.67 x the photons per
                                          # second at 0.2 % more per-pixel noise, profiles/r03/weight_roulette_sweep_mv9.log); 0 = off

    def __post_init__(self):
        self.zgrd  = np.ascontiguousarray(self.zgrd, dtype=np.float64)
        nz = self.zgrd.size - 1
        self.ext1d = _f32(np.atleast_2d(self.ext1d))
        self.omg1d = _f32(np.atleast_2d(self.omg1d))
        self.apf1d = _f32(np.atleast_2d(self.apf1d))
        self.abs1d = _f32(self.abs1d)
        if self.ext1d.shape[1] != nz or self.omg1d.shape != self.ext1d.shape or \
           self.apf1d.shape != self.ext1d.shape or self.abs1d.shape != (nz,):
            raise ValueError('Error [Scene]: 1-D profiles do not match the %d layers of <zgrd>.' % nz)
        if np.any(np.diff(self.zgrd) <= 0.0):
            raise ValueError('Error [Scene]: <zgrd> must be strictly ascending.')
        if self.nz3 > 0:
            shp = (self.nz3, self.ny, self.nx)
            self.extp = _f32(self.extp); self.omgp = _f32(self.omgp); self.apfp = _f32(self.apfp)
            if self.extp.ndim == 3:
                self.extp = self.extp[None]; self.omgp = self.omgp[None]; self.apfp = self.apfp[None]
            if self.extp.shape[1:] != shp or self.omgp.shape != self.extp.shape or self.apfp.shape != self.extp.shape:
                raise ValueError('Error [Scene]: 3-D arrays must be (np3d, nz3, ny, nx) = (*, %d, %d, %d).' % shp)
            if self.abst is not None:
                self.abst = _f32(self.abst)
                if self.abst.shape != shp:
                    raise ValueError('Error [Scene]: <abst> must be (nz3, ny, nx).')
            if self.iz3l < 1 or self.iz3l - 1 + self.nz3 > nz:
                raise ValueError('Error [Scene]: 3-D layers %d..%d do not fit the %d layers of the 1-D grid.' % (self.iz3l, self.iz3l+self.nz3-1, nz))
        if self.pha is not None:
            self.ang = _f32(self.ang)
            self.pha = _f32(np.atleast_2d(self.pha))
            if self.pha.shape[1] != self.ang.size:
                raise ValueError('Error [Scene]: <pha> must be (npf, nang).')
        self.sfc_param = _f32(np.resize(np.asarray(self.sfc_param, dtype=np.float32), 5)) if np.size(self.sfc_param) == 5 \
                         else _f32(np.concatenate([np.ravel(self.sfc_param), np.zeros(5)])[:5])
        if self.jsfc is not None:
            self.jsfc = _f32(self.jsfc)
            self.psfc = _f32(self.psfc)
            if self.psfc.shape != (5,) + self.jsfc.shape:
                raise ValueError('Error [Scene]: <psfc> must be (5, nyb, nxb).')
        if self.rad_kind == 1:
            n = len(self.view_the)
            for name, default in (('cam_xpos', 0.5), ('cam_ypos', 0.5), ('cam_psi', 0.0), ('cam_qmax', 180.0), ('cam_umax', 180.0),
                                  ('cam_vmax', 180.0), ('cam_apsize', 0.0)):
                v = list(np.resize(np.asarray(getattr(self, name) if len(getattr(self, name)) else [default], dtype=np.float64), n))
                setattr(self, name, v)
            if self.cam_method not in (0, 1):
                raise ValueError('Error [Scene]: <cam_method=%s> (Rad_mbwd) must be 0 (forward) or 1 (backward).' % self.cam_method)
            if self.cam_mpmap not in (1, 2) or self.cam_mrproj not in (0, 1):
                raise ValueError('Error [Scene]: <cam_mpmap=%s> (Rad_mpmap) must be 1 or 2 and <cam_mrproj=%s> (Rad_mrproj) 0 or 1.'
                                 % (self.cam_mpmap, self.cam_mrproj))
        elif self.rad_kind != 2:
            raise ValueError('Error [Scene]: <rad_kind=%s> (Rad_mrkind) must be 1 or 2.' % self.rad_kind)
        elif self.cam_method != 0:
            raise ValueError('Error [Scene]: <cam_method=%s> (Rad_mbwd) belongs to cameras and point radiometers (<rad_kind=1>).' % self.cam_method)
        if self.view_method not in (0, 1) or isinstance(self.view_method, float):
            raise ValueError('Error [Scene]: <view_method=%s> (Rad_mvbwd) must be 0 (forward) or 1 (backward).' % (self.view_method,))
        if self.view_method == 1 and self.rad_kind != 2:
            raise ValueError('Error [Scene]: <view_method=1> (Rad_mvbwd) belongs to satellite views (<rad_kind=2>); cameras and point radiometers '
                             'have <cam_method> (Rad_mbwd).')
        if self.cam_weights not in (0, 1):
            raise ValueError('Error [Scene]: <cam_weights=%s> (Rad_mwgt) must be 0 or 1.' % (self.cam_weights,))
        if self.cam_weights == 1 and not (self.rad_kind == 1 and self.cam_method == 1):
            raise ValueError('Error [Scene]: <cam_weights=1> (Rad_mwgt) needs the backward route (<rad_kind=1>, <cam_method=1>).')
        if self.view_profiles not in (0, 1) or isinstance(self.view_profiles, float):
            raise ValueError('Error [Scene]: <view_profiles=%s> (Rad_mvprf) must be 0 or 1.' % (self.view_profiles,))
        if self.view_profiles == 1 and not (self.rad_kind == 2 and self.view_method == 1):
            raise ValueError('Error [Scene]: <view_profiles=1> (Rad_mvprf) needs the backward route for satellite views (<rad_kind=2>, <view_method=1>).')
        if self.pixel_errors not in (0, 1) or isinstance(self.pixel_errors, float):
            raise ValueError('Error [Scene]: <pixel_errors=%s> (Rad_mserr) must be 0 or 1.' % (self.pixel_errors,))
        if self.pixel_errors == 1 and not ((self.rad_kind == 1 and self.cam_method == 1) or (self.rad_kind == 2 and self.view_method == 1)):
            raise ValueError('Error [Scene]: <pixel_errors=1> (Rad_mserr) needs a backward route (<cam_method=1> or <view_method=1>): on a forward '
                             'route one photon\'s contributions land in many pixels.')
        if self.pixel_errors == 1 and (self.cam_weights == 1 or self.view_profiles == 1):
            raise ValueError('Error [Scene]: <pixel_errors=1> (Rad_mserr) is not served together with <cam_weights=1> (Rad_mwgt) or '
                             '<view_profiles=1> (Rad_mvprf).')
        if self.view_sunlight not in (0, 1) or isinstance(self.view_sunlight, float):
            raise ValueError('Error [Scene]: <view_sunlight=%s> (Rad_mvsun) must be 0 or 1.' % (self.view_sunlight,))
        if self.view_sunlight == 1:
            why = 'the backward route for satellite views (<rad_kind=2>, <view_method=1>, Rad_mvbwd=1)' if not (self.rad_kind == 2 and self.view_method == 1) \
                  else 'a solar+thermal source (<src_mtype=2>): the switch belongs to the mixed source, a pure solar image is a mixed job with a cold atmosphere' \
                  if self.src_mtype != 2 \
                  else 'a job without <view_profiles=1> (Rad_mvprf): the weighting functions are per unit Planck radiance, and the sun has no row' \
                  if self.view_profiles == 1 \
                  else 'a sun from above (<src_the> - <src_qmax>/2 > 90)' if not (float(self.src_the) - 0.5*max(float(self.src_qmax), 0.0) > 90.0) else None
            if why:
                raise ValueError('Error [Scene]: <view_sunlight=1> (Rad_mvsun) needs %s.' % why)
        if self.view_columns not in (0, 1) or isinstance(self.view_columns, float):
            raise ValueError('Error [Scene]: <view_columns=%s> (Rad_mvcol) must be 0 or 1.' % (self.view_columns,))
        if self.view_columns == 1:
            why = 'the backward route for satellite views (<rad_kind=2>, <view_method=1>, Rad_mvbwd=1): cameras and point radiometers fan out over ' \
                  'the columns' if not (self.rad_kind == 2 and self.view_method == 1) \
                  else 'independent columns or partial 3-D (<solver=2> or <solver=1>): the 3-D solver runs without the switch' \
                  if int(self.solver) == SOLVER_3D else None
            if why:
                raise ValueError('Error [Scene]: <view_columns=1> (Rad_mvcol) needs %s.' % why)
        if self.src_mtype in (2, 3):
            if self.src_mtype == 2:
                if self.src_fsol is None or not (float(self.src_fsol) >= 0.0) or not np.isfinite(float(self.src_fsol)):
                    raise ValueError('Error [Scene]: a solar+thermal source (Src_mtype=2) needs the solar irradiance <Src_fsol> >= 0 [W m-2 um-1], got %s.'
                                     % self.src_fsol)
                self.src_fsol = float(self.src_fsol)
            if self.src_wlen is None or not (float(self.src_wlen) > 0.0):
                raise ValueError('Error [Scene]: a thermal source (Src_mtype=%d) needs the band-centre wavelength <Src_wlen> [um].' % self.src_mtype)
            self.tmp1d = _f32(np.ravel(self.tmp1d)) if self.tmp1d is not None else None
            if self.tmp1d is None or self.tmp1d.size != nz + 1:
                raise ValueError('Error [Scene]: a thermal source needs the %d interface temperatures <Atm_tmp1d> (nz+1), got %s.'
                                 % (nz+1, None if self.tmp1d is None else self.tmp1d.size))
            if self.tmpa3d is not None:
                self.tmpa3d = _f32(self.tmpa3d)
                if self.tmpa3d.shape != (self.nz3, self.ny, self.nx):
                    raise ValueError('Error [Scene]: <tmpa3d> must be (nz3, ny, nx).')
            if self.tmps2d is not None:
                self.tmps2d = _f32(self.tmps2d)
                if self.jsfc is None or self.tmps2d.shape != self.jsfc.shape:
                    raise ValueError('Error [Scene]: <tmps2d> must have the (nyb, nxb) shape of a 2-D surface.')
        elif self.src_mtype != 1:
            raise ValueError('Error [Scene]: <Src_mtype=%s> is not supported (1: solar, 2: solar+thermal, 3: thermal).' % self.src_mtype)

    # convenient sizes
    @property
    def nz(self):
        return self.zgrd.size - 1

    @property
    def np1d(self):
        return self.ext1d.shape[0]

    @property
    def np3d(self):
        return 0 if self.nz3 == 0 else self.extp.shape[0]

    @property
    def npf(self):
        return 0 if self.pha is None else self.pha.shape[0]

    @property
    def nview(self):
        return len(self.view_the)

    @property
    def mu0(self):
        return abs(np.cos(np.deg2rad(self.src_the)))

    # ------------------------------------------------------------------------------------------
    @classmethod
    def from_nml(cls, nml, fdir='.', solver=SOLVER_3D):

        """
        Build a Scene from a flat namelist dictionary {key: value} as assembled by `mcarats_ng`
        (reference: er3t/rtm/mca/mcarats.py:234-414) -- or parsed back from an input file -- with
        side-file paths taken relative to <fdir> (mcarats.py:323,352,406).
        """

        def get(key, default=None):
            return nml[key] if key in nml and nml[key] is not None else default

        zgrd = np.asarray(get('Atm_zgrd0'), dtype=np.float64)
        nz   = int(get('Atm_nz', zgrd.size-1))
        zgrd = zgrd[:nz+1]
        np1d = int(get('Atm_np1d', 1))

        def col(base, ip, default):
            # indexed keys look like 'Atm_ext1d(1:, 2)' (mca_atm.py:91-102,135-137)
            for key in nml:
                m = re.match(r'%s\(\s*1:\s*,\s*(\d+)\s*\)' % base, key)
                if m and int(m.group(1)) == ip+1:
                    return np.resize(np.asarray(nml[key], dtype=np.float64), nz)
            if ip == 0 and base in nml and nml[base] is not None:
                return np.resize(np.asarray(nml[base], dtype=np.float64), nz)
            return np.full(nz, default)

        ext1d = np.stack([col('Atm_ext1d', ip, 0.0) for ip in range(np1d)])
        omg1d = np.stack([col('Atm_omg1d', ip, 1.0) for ip in range(np1d)])
        apf1d = np.stack([col('Atm_apf1d', ip, -1.0) for ip in range(np1d)])
        abs1d = col('Atm_abs1d', 0, 0.0)
        for base, arr in (('Atm_fext1d', ext1d),):
            fac = get(base)
            if fac is not None:
                arr *= np.resize(np.asarray(fac, dtype=np.float64), np1d)[:, None]
        abs1d = abs1d * float(get('Atm_fabs1d', 1.0))

        kw = dict(zgrd=zgrd, ext1d=ext1d, omg1d=omg1d, apf1d=apf1d, abs1d=abs1d)

        nx = int(get('Atm_nx', 1)); ny = int(get('Atm_ny', 1))
        kw.update(nx=nx, ny=ny, dx=float(get('Atm_dx', 1.0e4)), dy=float(get('Atm_dy', 1.0e4)))

        nz3 = int(get('Atm_nz3', 0))
        if nz3 > 0:
            np3d = int(get('Atm_np3d', 1))
            fname = os.path.join(fdir, get('Atm_inpfile'))
            nvox = nx*ny*nz3
            raw = np.fromfile(fname, dtype='<f4')
            if raw.size != nvox*(2+3*np3d):
                raise OSError('Error [Scene]: <%s> holds %d values, expected %d.' % (fname, raw.size, nvox*(2+3*np3d)))
            blocks = raw.reshape(2+3*np3d, nz3, ny, nx)
            fext3d = np.resize(np.asarray(get('Atm_fext3d', 1.0), dtype=np.float32), np3d)
            kw.update(nz3=nz3, iz3l=int(get('Atm_iz3l', 1)), tmpa3d=blocks[0],
                      abst=blocks[1]*np.float32(get('Atm_fabs3d', 1.0)),
                      extp=blocks[2::3]*fext3d[:, None, None, None], omgp=blocks[3::3], apfp=blocks[4::3])

        npf = int(get('Sca_npf', 0))
        if npf > 0:
            nang  = int(get('Sca_nangi'))
            fname = os.path.join(fdir, get('Sca_inpfile'))
            raw   = np.fromfile(fname, dtype='<f4')
            if raw.size < nang*(1+npf):
                raise OSError('Error [Scene]: <%s> holds %d values, expected %d.' % (fname, raw.size, nang*(1+npf)))
            kw.update(ang=raw[:nang], pha=raw[nang:nang*(1+npf)].reshape(npf, nang))

        if get('Sfc_inpfile') is not None and int(get('Sfc_nxb', 0)) > 0:
            nxb = int(get('Sfc_nxb')); nyb = int(get('Sfc_nyb'))
            raw = np.fromfile(os.path.join(fdir, get('Sfc_inpfile')), dtype='<f4')
            if raw.size != 7*nxb*nyb:
                raise OSError('Error [Scene]: surface file holds %d values, expected %d.' % (raw.size, 7*nxb*nyb))
            blocks = raw.reshape(7, nyb, nxb)
            kw.update(jsfc=blocks[1], psfc=blocks[2:7], tmps2d=blocks[0])
        else:
            param = np.zeros(5, dtype=np.float32)
            if get('Sfc_param') is not None:
                p = np.ravel(np.asarray(get('Sfc_param'), dtype=np.float32))
                param[:p.size] = p[:5]
            for i in range(5):
                key = 'Sfc_param(%d)' % (i+1)
                if key in nml and nml[key] is not None:
                    param[i] = nml[key]
            kw.update(sfc_mtype=int(get('Sfc_mtype', 1)), sfc_param=param)

        kw.update(src_flx=float(get('Src_flx', 1.0)), src_qmax=float(get('Src_qmax', 0.0)),
                  src_the=float(get('Src_the', 120.0)), src_phi=float(get('Src_phi', 0.0)))

        mtype = int(get('Src_mtype', 1))
        if mtype in (2, 3):
            if mtype == 2:
                if get('Src_fsol') is None:
                    raise OSError('Error [Scene]: a solar+thermal job (<Src_mtype=2>) needs <Src_fsol>, the solar irradiance at the top of the '
                                  'atmosphere in W m-2 um-1.')
                kw.update(src_fsol=float(np.ravel(get('Src_fsol'))[0]))
            if get('Src_wlen') is None:
                raise OSError('Error [Scene]: a thermal job (Src_mtype=%d) needs <Src_wlen>, the band-centre wavelength in micrometres.' % mtype)
            tmp = np.ravel(np.asarray(get('Atm_tmp1d', []), dtype=np.float64))
            if tmp.size != nz + 1:
                raise OSError('Error [Scene]: a thermal job needs the %d INTERFACE temperatures <Atm_tmp1d> (nz+1); %d values (%s) are ambiguous.'
                              % (nz+1, tmp.size, 'nz: layer temperatures' if tmp.size == nz else 'neither nz nor nz+1'))
            kw.update(src_mtype=mtype, src_wlen=float(np.ravel(get('Src_wlen'))[0]), tmp1d=tmp)
        elif mtype != 1:
            raise OSError('Error [Scene]: <Src_mtype=%d> is not supported (1: solar, 2: solar+thermal, 3: thermal).' % mtype)
        else:
            kw.pop('tmpa3d', None); kw.pop('tmps2d', None)

        mtarget = int(get('Wld_mtarget', 1))
        # (a key of this project: backward Monte Carlo for the cameras and point radiometers of a thermal job)
        mbwd = float(np.ravel(get('Rad_mbwd', 0))[0])
        if mbwd not in (0.0, 1.0):
            raise OSError('Error [Scene]: <Rad_mbwd=%g> is not supported (0: forward, 1: backward Monte Carlo).' % mbwd)
        if mbwd == 1.0 and not (mtype == 3 and mtarget == 2 and int(get('Rad_mrkind', 2)) == 1):
            raise OSError('Error [Scene]: <Rad_mbwd=1> (backward Monte Carlo) belongs to the cameras and point radiometers (<Rad_mrkind=1>) of a '
                          'thermal job (<Src_mtype=3>).')
        # (a key of this project: backward Monte Carlo for the satellite views of a thermal job)
        mvbwd = float(np.ravel(get('Rad_mvbwd', 0))[0])
        if mvbwd not in (0.0, 1.0):
            raise OSError('Error [Scene]: <Rad_mvbwd=%g> is not supported (0: forward, 1: backward Monte Carlo for satellite views).' % mvbwd)
        # (a key of this project: the sunlight term of that route, which lets it serve a solar+thermal job)
        mvsun = float(np.ravel(get('Rad_mvsun', 0))[0])
        if mvsun not in (0.0, 1.0):
            raise OSError('Error [Scene]: <Rad_mvsun=%g> is not supported (0: off, 1: the sunlight term of the backward satellite views).' % mvsun)
        if mvsun == 1.0 and (int(get('Rad_mrkind', 2)) != 2 or float(np.ravel(get('Rad_mwgt', 0))[0]) == 1.0):
            raise OSError('Error [Scene]: <Rad_mvsun=1> (sunlight on the backward satellite views) belongs to satellite views (<Rad_mrkind=2>) '
                          'without emission weights (<Rad_mwgt=1>): cameras and point radiometers of a mixed job are not served backwards, and '
                          'the sun is no cell.')
        if mvsun == 1.0 and not (mvbwd == 1.0 and mtype == 2):
            raise OSError('Error [Scene]: <Rad_mvsun=1> (sunlight on the backward satellite views) needs <Rad_mvbwd=1> and the solar+thermal source '
                          '(<Src_mtype=2>); a pure solar image is a mixed job with a cold atmosphere.')
        # (a key of this project: that route under independent columns and partial 3-D, a history keeps its column)
        mvcol = float(np.ravel(get('Rad_mvcol', 0))[0])
        if mvcol not in (0.0, 1.0):
            raise OSError('Error [Scene]: <Rad_mvcol=%g> is not supported (0: off, 1: the backward satellite views under independent columns and '
                          'partial 3-D).' % mvcol)
        if mvcol == 1.0 and (int(get('Rad_mrkind', 2)) != 2 or float(np.ravel(get('Rad_mwgt', 0))[0]) == 1.0):
            raise OSError('Error [Scene]: <Rad_mvcol=1> (column histories of the backward satellite views) belongs to satellite views '
                          '(<Rad_mrkind=2>) without emission weights (<Rad_mwgt=1>): cameras and point radiometers fan out over the columns.')
        if mvcol == 1.0 and mvbwd != 1.0:
            raise OSError('Error [Scene]: <Rad_mvcol=1> (column histories of the backward satellite views) needs the backward route for satellite '
                          'views (<Rad_mvbwd=1>).')
        if mvcol == 1.0 and int(solver) == SOLVER_3D:
            raise OSError('Error [Scene]: <Rad_mvcol=1> (column histories of the backward satellite views) belongs to independent columns and '
                          'partial 3-D (solver 2 / 1): the 3-D solver runs without the switch.')
        if mvbwd == 1.0 and not ((mtype == 3 or (mtype == 2 and mvsun == 1.0)) and mtarget == 2 and int(get('Rad_mrkind', 2)) == 2
                                 and (int(solver) == SOLVER_3D or mvcol == 1.0)):
            raise OSError('Error [Scene]: <Rad_mvbwd=1> (backward Monte Carlo) belongs to the satellite views (<Rad_mrkind=2>) of a thermal radiance '
                          'job (<Src_mtype=3>, <Wld_mtarget=2>) under the 3-D solver (a solar+thermal job, <Src_mtype=2>, with <Rad_mvsun=1>).')
        # (a key of this project: per-cell emission weights of the backward route)
        mwgt = float(np.ravel(get('Rad_mwgt', 0))[0])
        if mwgt not in (0.0, 1.0):
            raise OSError('Error [Scene]: <Rad_mwgt=%g> is not supported (0: off, 1: per-cell emission weights).' % mwgt)
        if mwgt == 1.0 and mbwd != 1.0:
            raise OSError('Error [Scene]: <Rad_mwgt=1> (emission weights) needs the backward route (<Rad_mbwd=1>).')
        # (a key of this project: per-layer profiles of the backward route's satellite views)
        mvprf = float(np.ravel(get('Rad_mvprf', 0))[0])
        if mvprf not in (0.0, 1.0):
            raise OSError('Error [Scene]: <Rad_mvprf=%g> is not supported (0: off, 1: per-layer weighting functions).' % mvprf)
        if mvprf == 1.0 and mvbwd != 1.0:
            raise OSError('Error [Scene]: <Rad_mvprf=1> (view profiles) needs the backward route for satellite views (<Rad_mvbwd=1>).')
        if mvprf == 1.0 and mvsun == 1.0:
            raise OSError('Error [Scene]: <Rad_mvprf=1> (view profiles) is not served together with <Rad_mvsun=1>: the weighting functions are per '
                          'unit Planck radiance, and the sun has no row.')
        # (a key of this project: per-pixel standard errors of the backward routes)
        mserr = float(np.ravel(get('Rad_mserr', 0))[0])
        if mserr not in (0.0, 1.0):
            raise OSError('Error [Scene]: <Rad_mserr=%g> is not supported (0: off, 1: per-pixel standard errors).' % mserr)
        if mserr == 1.0 and mbwd != 1.0 and mvbwd != 1.0:
            raise OSError('Error [Scene]: <Rad_mserr=1> (pixel errors) needs a backward route (<Rad_mbwd=1> or <Rad_mvbwd=1>): on a forward route '
                          'one photon\'s contributions land in many pixels.')
        if mserr == 1.0 and (mwgt == 1.0 or mvprf == 1.0):
            raise OSError('Error [Scene]: <Rad_mserr=1> (pixel errors) is not served together with <Rad_mwgt=1> or <Rad_mvprf=1>.')
        if mtarget == 2:
            nrad = int(get('Rad_nrad', 1))
            the  = np.resize(np.asarray(get('Rad_the', 180.0), dtype=np.float64), nrad)
            phi  = np.resize(np.asarray(get('Rad_phi', 0.0), dtype=np.float64), nrad)
            zloc = np.resize(np.asarray(get('Rad_zloc', 0.0), dtype=np.float64), nrad)
            kw.update(target=TARGET_RADIANCE, view_the=list(the), view_phi=list(phi), view_zloc=list(zloc),
                      zref=float(get('Rad_zref', 0.0)), nxr=int(get('Rad_nxr', 1)), nyr=int(get('Rad_nyr', 1)))
            mrkind = int(get('Rad_mrkind', 2))
            if mrkind == 1:
                mpmap, mrproj = int(get('Rad_mpmap', 1)), int(get('Rad_mrproj', 0))
                if mpmap not in (1, 2):
                    raise OSError('Error [Scene]: <Rad_mpmap=%d> is not supported for <Rad_mrkind=1> (1: polar, 2: rectangular).' % mpmap)
                if mrproj not in (0, 1):
                    raise OSError('Error [Scene]: <Rad_mrproj=%d> is not supported (0: mean radiance, 1: cosine-weighted).' % mrproj)
                def per_view(key, default):
                    return list(np.resize(np.asarray(get(key, default), dtype=np.float64), nrad))
                kw.update(rad_kind=1, cam_xpos=per_view('Rad_xpos', 0.5), cam_ypos=per_view('Rad_ypos', 0.5),
                          cam_psi=per_view('Rad_psi', 0.0), cam_qmax=per_view('Rad_qmax', 180.0), cam_umax=per_view('Rad_umax', 180.0),
                          cam_vmax=per_view('Rad_vmax', 180.0), cam_apsize=per_view('Rad_apsize', 0.0), cam_mpmap=mpmap, cam_mrproj=mrproj,
                          cam_method=int(mbwd), cam_weights=int(mwgt), pixel_errors=int(mserr))
                # (a key of this project: the periodic images of a sensor the job asks for; without it the route's default, cam_images = -1)
                if get('Rad_nimg') is not None:
                    nimg = float(np.ravel(get('Rad_nimg'))[0])
                    if nimg != int(nimg) or not 0 <= int(nimg) <= 8:
                        raise OSError('Error [Scene]: <Rad_nimg=%g> must be an integer from 0 to 8.' % nimg)
                    kw.update(cam_images=int(nimg))
            elif mrkind != 2:
                raise OSError('Error [Scene]: <Rad_mrkind=%d> is not supported (1: camera, 2: satellite).' % mrkind)
            else:
                kw.update(view_method=int(mvbwd), view_profiles=int(mvprf), pixel_errors=int(mserr), view_sunlight=int(mvsun), view_columns=int(mvcol))
        elif mtarget == 1:
            mhrt = int(get('Flx_mhrt', 0) or 0)
            if mhrt == 2 and mtype not in (2, 3):
                raise OSError('Error [Scene]: <Flx_mhrt=2> is the NET heating rate of a thermal job (Src_mtype=3); nothing emits in a solar job: use <Flx_mhrt=1>.')
            # (Flx_mhrt = 1 with the thermal source stays refused by mca_exe: absorbed or net is what is ambiguous about it)
            kw.update(target=TARGET_FLUX | (TARGET_HEAT if (mhrt == 1 or (mhrt == 2 and mtype in (2, 3))) else 0))
            mhest = int(get('Flx_mhest', 0) or 0)
            if mhest not in (0, 1):
                raise OSError('Error [Scene]: <Flx_mhest=%d> is not supported (0: collision estimator, 1: path-length estimator).' % mhest)
            kw.update(heat_estimator=mhest)
        else:
            raise OSError('Error [Scene]: <Wld_mtarget=%d> is not supported.' % mtarget)

        kw.update(solver=int(solver), wmin=float(get('Pho_wmin', 0.2)), wfac=float(get('Pho_wfac', 1.0)))

        return cls(**kw)
