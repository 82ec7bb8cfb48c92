"""
Cameras and point radiometers of thermal jobs (Src_mtype = 3, Rad_mrkind = 1) without a GPU: the namelist key Rad_nimg
through mca_exe's checks and Scene.from_nml, the job files mcarats_ng writes (and that solar camera job files are unchanged), mca_out_ng
on hand-made output files, and the float64 reference of tests/test_gpu_thermal_camera.py against the closed form of a homogeneous slab.
"""

import contextlib
import dataclasses
import io
import os

import numpy as np
import pytest

import er3t_amd.rtm.mca as mca
from er3t_amd.rtm.mca.mca_exe import _check_supported, thermal_heating
from er3t_amd.rtm.mca.mca_out import mca_out_write
from er3t_amd.scene import Scene, TARGET_RADIANCE
from er3t_amd.synth import atm_synth, abs_synth
from er3t_amd.thermal import planck, brightness_temperature
from tests import thermal_camera_ref as ref
from tests.golden import inputs as gin


def _nml(nz=4, **kw):
    nml = {'Wld_mtarget': 2, 'Rad_mrkind': 1, 'Rad_nimg': 2, 'Atm_nz': nz, 'Atm_zgrd0': np.arange(nz+1)*1000.0, 'Src_mtype': 3, 'Src_wlen': 11.0,
           'Atm_tmp1d': np.linspace(290.0, 230.0, nz+1), 'Sfc_mtype': 1}
    nml.update(kw)
    return {k: v for k, v in nml.items() if v is not None}


def test_rad_nimg_opens_thermal_cameras():
    for n in (0, 2, 8):
        _check_supported(_nml(Rad_nimg=n))
    _check_supported(_nml(Rad_mpmap=2, Rad_mrproj=1))
    with pytest.raises(OSError) as err:
        _check_supported(_nml(Rad_nimg=None))
    assert 'Rad_nimg' in str(err.value) and 'all-sky' in str(err.value)
    for bad in (-1, 9, 1.5):
        with pytest.raises(OSError) as err:
            _check_supported(_nml(Rad_nimg=bad))
        assert 'Rad_nimg' in str(err.value)
    # solar+thermal cameras stay refused, with or without the key
    for kw in (dict(), dict(Rad_nimg=None)):
        with pytest.raises(OSError) as err:
            _check_supported(_nml(Src_mtype=2, Src_fsol=10.0, **kw))
        assert 'all-sky' in str(err.value)
    # a solar camera job may carry the key too, within its range
    solar = dict(Src_mtype=1, Src_wlen=None, Atm_tmp1d=np.linspace(290.0, 230.0, 4))
    _check_supported(_nml(**solar)); _check_supported(_nml(Rad_nimg=None, **solar))
    with pytest.raises(OSError):
        _check_supported(_nml(Rad_nimg=12, **solar))
    # several ranks take such jobs one by one (the batched route's normalisation is the solar one)
    assert thermal_heating(_nml()) and not thermal_heating(_nml(**solar)) and not thermal_heating(_nml(Rad_mrkind=2, Rad_nimg=None))


def _objects(wvl):
    atm = atm_synth(np.arange(17)*1.0)
    ab = abs_synth(wvl, atm, Ng=2)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
    return atm, ab, a1


def _write(a1, ab, fdir, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return mca.mcarats_ng(atm_1ds=[a1], Ng=2, target='radiance', surface_albedo=0.03, fdir=fdir, Nrun=1, photons=1e4,
                              weights=ab.coef['weight']['data'], mp_mode='batch', overwrite=True, date=gin.DATE, quiet=True, **kw)


SENSORS = {'all-sky': dict(sensor_type='all-sky', sensor_altitude=0.0, sensor_zenith_angle=180.0),
           'irradiance': dict(sensor_type='irradiance', sensor_xpos=[0.2, 0.7], sensor_ypos=0.5, sensor_altitude=10.0, sensor_zenith_angle=[0.0, 180.0]),
           'actinic': dict(sensor_type='actinic', sensor_altitude=500.0, sensor_zenith_angle=0.0)}


@pytest.mark.parametrize('kind', sorted(SENSORS))
def test_thermal_sensor_job_files_parse_back(tmp_path, kind):
    atm, ab, a1 = _objects(11000.0)
    for images, want in ((None, 2), (0, 0), (5, 5)):
        m = _write(a1, ab, str(tmp_path/('th%s' % images)), source='thermal', camera_images=images, **SENSORS[kind])
        nml = mca.mca_inp_read(m.fnames_inp[0][0])
        assert nml['Src_mtype'] == 3 and nml['Rad_mrkind'] == 1 and nml['Rad_nimg'] == want
        _check_supported(nml)
        sc = Scene.from_nml(nml, str(tmp_path), solver=0)
        assert sc.src_mtype == 3 and sc.rad_kind == 1 and sc.cam_images == want
        assert sc.cam_mpmap == (1 if kind == 'all-sky' else 2) and sc.cam_mrproj == (1 if kind == 'irradiance' else 0)
        assert thermal_heating(nml)
    with pytest.raises(OSError) as err:
        _write(a1, ab, str(tmp_path/'mix'), source='solar+thermal', **SENSORS[kind])
    assert 'solar+thermal' in str(err.value)
    for bad in (-1, 9, 2.5):
        with pytest.raises(OSError):
            _write(a1, ab, str(tmp_path/'bad'), source='thermal', camera_images=bad, **SENSORS[kind])


@pytest.mark.parametrize('kind', ['all-sky', 'irradiance'])
def test_solar_sensor_job_files_do_not_change(tmp_path, kind):
    """without <camera_images> a solar camera job file carries no Rad_nimg: the text is the text without the keyword, and with it the one
    line more; Scene.from_nml maps the key for a solar job too and leaves cam_images at -1 without it"""
    atm, ab, a1 = _objects(650.0)
    m0 = _write(a1, ab, str(tmp_path/'a'), **SENSORS[kind])
    m1 = _write(a1, ab, str(tmp_path/'b'), camera_images=3, **SENSORS[kind])
    strip = lambda s: [l for l in s.splitlines() if 'Wld_jseed' not in l]
    t0, t1 = strip(open(m0.fnames_inp[0][0]).read()), strip(open(m1.fnames_inp[0][0]).read())
    assert not any('Rad_nimg' in l for l in t0)
    assert [l for l in t1 if 'Rad_nimg' not in l] == t0 and sum('Rad_nimg' in l for l in t1) == 1
    # ... and is what the catalogue's other keys alone give: the group of the new key holds the keys it held
    rad = t0[t0.index('&mcarRad_nml_job'):]
    assert [l.split('=')[0].strip() for l in rad[1:rad.index('/')]][-1].startswith('Rad_')
    assert Scene.from_nml(mca.mca_inp_read(m0.fnames_inp[0][0]), str(tmp_path), solver=0).cam_images == -1
    assert Scene.from_nml(mca.mca_inp_read(m1.fnames_inp[0][0]), str(tmp_path), solver=0).cam_images == 3


class _Files:
    """what mca_out_ng reads of a thermal mcarats_ng object"""
    def __init__(self, fdir, Nrun, Ng, sensor_type, nview, wlen_um):
        self.Nrun, self.Ng, self.target, self.source, self.wlen_um = Nrun, Ng, 'radiance', 'thermal', wlen_um
        self.sensor_type, self.Nview = sensor_type, nview
        os.makedirs(fdir, exist_ok=True)
        self.fnames_out = [['%s/r%02d.g%03d.out.bin' % (fdir, ir, ig) for ig in range(Ng)] for ir in range(Nrun)]
        self.photons = np.full(Nrun*Ng, 1000)
        self.fused = None


def test_mca_out_ng_on_thermal_sensor_files(tmp_path):
    Ng, Nrun, wl = 3, 2, 11.0
    rng = np.random.default_rng(5)
    ab = abs_synth(11000.0, atm_synth(np.arange(4)*1.0), Ng=Ng)
    w = ab.coef['weight']['data']
    # an all-sky image: the thermal g-sum, and its brightness temperature
    m = _Files(str(tmp_path/'sky'), Nrun, Ng, 'all-sky', 1, wl)
    rad = {}
    for ir in range(Nrun):
        for ig in range(Ng):
            rad[ir, ig] = planck(wl, rng.uniform(200.0, 290.0, (6, 5, 1, 1))).astype(np.float32)
            mca_out_write(m.fnames_out[ir][ig], [('rad', 'radiance', rad[ir, ig])])
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='all', squeeze=True, quiet=True).data
    for ir in range(Nrun):
        want = np.zeros((6, 5), dtype=np.float32)
        for ig in range(Ng):
            want += rad[ir, ig][:, :, 0, 0]*np.float32(w[ig]*1.0e-3)
        assert np.array_equal(out['rad']['data'][..., ir], want)
    assert np.allclose(planck(wl, out['bt']['data']), out['rad']['data']*1.0e3, rtol=2e-6)
    mean = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    assert np.allclose(brightness_temperature(wl, mean['rad']['data']*1.0e3), mean['bt']['data'], rtol=1e-6)
    # radiometers: f = k x the g-sum of `rad`, k = pi (irradiance) or 2 pi (actinic); no direct part
    for kind, k in (('irradiance', np.pi), ('actinic', 2.0*np.pi)):
        mr = _Files(str(tmp_path/kind), Nrun, Ng, kind, 4, wl)
        vals = {}
        for ir in range(Nrun):
            for ig in range(Ng):
                vals[ir, ig] = rng.uniform(1.0, 9.0, (1, 1, 4, 1)).astype(np.float32)
                mca_out_write(mr.fnames_out[ir][ig], [('rad', 'radiance', vals[ir, ig]), ('rdir', 'direct', np.zeros_like(vals[ir, ig]))])
        o = mca.mca_out_ng(mca_obj=mr, abs_obj=ab, mode='all', squeeze=True, quiet=True).data
        for ir in range(Nrun):
            want = np.zeros(4, dtype=np.float32)
            for ig in range(Ng):
                want += vals[ir, ig][0, 0, :, 0]*np.float32(w[ig]*1.0e-3)
            assert np.array_equal(o['f']['data'][:, ir], want*np.float32(k)), kind
        assert np.all(o['f_direct']['data'] == 0.0) and np.array_equal(o['f']['data'], o['f_diffuse']['data'])
        om = mca.mca_out_ng(mca_obj=mr, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
        assert np.all(om['f_direct']['data'] == 0.0) and np.all(om['f_direct_std']['data'] == 0.0) and om['f']['data'].shape == (4,)
        assert np.allclose(om['f']['data'], o['f']['data'].mean(axis=-1), rtol=1e-6)


# ---- the float64 reference of the GPU tests, on its own -----------------------------------------------------------------------------------

def _slab(kappa=1.0e-3, T=280.0, albedo=0.0, t_sfc=None, n=4):
    """a homogeneous absorbing slab, 1 km thick, isothermal: two 1-D layers and two layers of voxels holding the same medium"""
    nz, dz = 4, 250.0
    absk = np.array([kappa, 0.0, 0.0, kappa])
    v = np.full((1, 2, n, n), kappa, dtype=np.float32)
    tl = np.full(nz+1, T)
    if t_sfc is not None:
        tl[0] = t_sfc        # (also shifts the lowest layer's mean: give that layer no absorber)
        absk[0] = 0.0
    return Scene(zgrd=np.arange(nz+1)*dz, ext1d=np.zeros(nz), omg1d=np.ones(nz), apf1d=np.full(nz, -1.0), abs1d=absk, nx=n, ny=n, dx=300.0,
                 dy=200.0, nz3=2, iz3l=2, extp=v, omgp=np.zeros_like(v), apfp=np.zeros_like(v), sfc_mtype=1, sfc_param=[albedo, 0, 0, 0, 0],
                 target=TARGET_RADIANCE, rad_kind=1, view_the=[0.0], view_phi=[0.0], view_zloc=[0.0], nxr=1, nyr=1, src_mtype=3, src_wlen=11.0,
                 tmp1d=tl, src_the=180.0, src_qmax=0.0, cam_mpmap=2, cam_mrproj=1, cam_umax=[90.0], cam_vmax=[180.0])


def test_reference_march_on_a_homogeneous_slab():
    """looking up through the slab from the ground: B (1 - exp(-tau / mu)) in every direction, whatever cells the line crosses; looking down
    from the top at a warm grey surface: the slab's emission, the surface's, and what the surface reflects of the slab's own downwelling"""
    sc = _slab()
    kap = float(np.float32(1.0e-3))                    # (the scene holds float32)
    B, tau = float(planck(11.0, 280.0)), 1000.0*kap
    mu = np.array([1.0, 0.7, 0.3, 0.05]); ph = np.array([0.3, 2.0, 4.0, 5.5])
    d = np.stack([np.sqrt(1.0-mu**2)*np.cos(ph), np.sqrt(1.0-mu**2)*np.sin(ph), mu], axis=-1)
    I = ref.march(sc, [410.0, 130.0, 0.0], d)
    assert np.allclose(I, B*(1.0-np.exp(-tau/mu)), rtol=1e-11)
    # a box: the line is cut where it leaves |dx| <= (N + 1/2) Lx or |dy| <= (N + 1/2) Ly, the optical depth up to there is what counts
    Ib = ref.march(sc, [410.0, 130.0, 0.0], d, nimg=0)
    with np.errstate(divide="ignore"):
        s_box = np.minimum(600.0/np.abs(d[:, 0]), 400.0/np.abs(d[:, 1]))
    want = B*(1.0-np.exp(-kap*np.minimum(s_box, 1000.0/mu)))
    assert np.allclose(Ib, want, rtol=1e-11) and np.any(Ib < 0.99*I)
    # the hemispheric irradiance by the pixel quadrature of a one-pixel irradiance sensor: pi B (1 - 2 E3(tau))
    from scipy.special import expn
    img = ref.rect_image(sc, 0, None, 24)
    assert img.shape == (1, 1) and abs(np.pi*img[0, 0]/(np.pi*B*(1.0-2.0*expn(3, tau)))-1.0) < 1e-6
    # looking down at a grey surface (albedo 0.2, 300 K) under the slab (its lowest quarter without absorber: tau 0.75)
    sg = dataclasses.replace(_slab(albedo=0.2, t_sfc=300.0), view_the=[180.0], view_zloc=[1000.0])
    Bs, t2 = float(planck(11.0, 300.0)), 750.0*kap
    refl = ref.surface_reflection(sg, 4, 24, 8)
    E = np.pi*B*(1.0-2.0*expn(3, t2))
    assert abs(refl(np.array([100.0]), np.array([700.0]))[0]/(0.2*E/np.pi)-1.0) < 1e-6
    dn = d*np.array([1.0, 1.0, -1.0])
    Id = ref.march(sg, [410.0, 130.0, 1000.0], dn, refl=refl)
    assert np.allclose(Id, B*(1.0-np.exp(-t2/mu))+(0.8*Bs+0.2*E/np.pi)*np.exp(-t2/mu), rtol=1e-6)
