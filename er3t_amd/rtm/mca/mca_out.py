"""
Solver outputs: reader of one out.bin (+ .ctl), and the reduction over g and runs.

Counterparts of the reference's `mca_out_raw` and `mca_out_ng` / `read_flux_mca_out` / `read_radiance_mca_out`
(er3t/rtm/mca/mca_out.py:16-103, 107-505), plus `mca_out_write`, which produces the files those readers parse
(the reference never writes them: its solver executable does).
"""

import os

import numpy as np

from er3t_amd.util import cal_sol_fac

__all__ = ['mca_out_raw', 'mca_out_ng', 'mca_out_write', 'read_flux_mca_out', 'read_radiance_mca_out', 'read_heating_mca_out',
           'read_radiometer_mca_out']


def mca_out_write(fname_bin, variables):

    """
    Write a solver output: <fname_bin> = float32 little-endian, every variable (nx, ny, nz, nt) in Fortran order
    one after the other; <fname_bin>.ctl = GrADS descriptor with the XDEF / YDEF / TDEF / VARS lines
    `mca_out_raw` reads (er3t/rtm/mca/mca_out.py:48-91).

    variables: list of (name, description, array) with array (nx, ny, nz) or (nx, ny, nz, nt)
    """

    arrays = []
    for name, desc, a in variables:
        a = np.asarray(a, dtype='<f4')
        if a.ndim == 3:
            a = a[..., np.newaxis]
        arrays.append((name, desc, a))
    nx, ny, _, nt = arrays[0][2].shape
    nzmax = max(a.shape[2] for _, _, a in arrays)

    with open(fname_bin, 'wb') as f:
        for _, _, a in arrays:
            a.ravel(order='F').tofile(f)

    lines = ['DSET ^%s' % os.path.basename(fname_bin),
             'TITLE er3t_amd solver output',
             'OPTIONS LITTLE_ENDIAN',
             'UNDEF -9.99E33',
             'XDEF %d LINEAR 1 1' % nx,
             'YDEF %d LINEAR 1 1' % ny,
             'ZDEF %d LINEAR 1 1' % nzmax,
             'TDEF %d LINEAR 00:00Z01JAN2000 1mn' % nt,
             'VARS %d' % len(arrays)]
    lines += ['%s %d 99 %s' % (name, a.shape[2], desc) for name, desc, a in arrays]
    lines += ['ENDVARS']
    with open(fname_bin+'.ctl', 'w') as f:
        f.write('\n'.join(lines)+'\n')


class mca_out_raw:

    """
    Read one solver output file using its .ctl descriptor.

    self.data: list (one entry per variable) of {'name', 'dims' [Nx, Ny, Nz, Nt], 'dims_info', 'data'}
    """

    def __init__(self, fname_bin):

        if not os.path.isfile(fname_bin):
            raise OSError('Error [mca_out_raw]: Cannot find <%s>.' % fname_bin)
        fname_ctl = fname_bin + '.ctl'
        if not os.path.isfile(fname_ctl):
            raise OSError('Error [mca_out_raw]: Cannot find <%s>.' % fname_ctl)

        self.fname_bin = fname_bin
        self.fname_ctl = fname_ctl
        self.data = []
        self.read_ctl()
        self.read_bin()

    def read_ctl(self):

        with open(self.fname_ctl, 'r') as f:
            lines = [l.strip() for l in f.readlines()]

        Nx = Ny = Nt = None
        start = 0
        for i, line in enumerate(lines):
            if 'XDEF' in line:
                Nx = int(line.replace('XDEF', '').replace('LINEAR', '').split()[0])
            elif 'YDEF' in line:
                Ny = int(line.replace('YDEF', '').replace('LINEAR', '').split()[0])
            elif 'TDEF' in line:
                Nt = int(line.replace('TDEF', '').split()[0])
            elif 'VARS' in line and 'ENDVARS' not in line:
                self.Nvar = int(line.replace('VARS', '').strip())
                for words in (l.split() for l in lines[i+1:i+1+self.Nvar]):
                    Nz = int(words[1])
                    size = Nx*Ny*Nz*Nt
                    self.data.append({'name': '%s (%s)' % (words[0], ' '.join(words[3:])), 'dims': [Nx, Ny, Nz, Nt],
                                      'dims_info': ['Nx', 'Ny', 'Nz', 'Nt'], 'Index_Start': start, 'Index_End': start+size})
                    start += size

    def read_bin(self, dtype='<f4'):
        raw = np.fromfile(self.fname_bin, dtype=dtype)
        for info in self.data:
            info['data'] = raw[info['Index_Start']:info['Index_End']].reshape(info['dims'], order='F')


# ----------------------------------------------------------------------------------------------
def g_factors(mca_obj, abs_obj, Nz):

    """
    factor[iz, ig] = sol_fac * solar[ig]*weight[ig]*slit[iz, ig] / sum_g(weight*slit[iz]) in float32, the slit
    function of the top level taken from the layer below it (reference: er3t/rtm/mca/mca_out.py:313-328)
    """

    weight = abs_obj.coef['weight']['data']
    source = getattr(mca_obj, 'source', 'solar')
    if source in ('thermal', 'solar+thermal'):
        # thermal source (Src_mtype = 3): every job's result is in W m-2 (sr-1) um-1 already -- no solar spectrum, no Earth-Sun
        # distance, no slit function: sum_g weight[ig] x_g, per nm like the solar output.  Solar+thermal (Src_mtype = 2): the same
        # float32 factors -- the job's own Src_fsol carries the solar spectrum and the Earth-Sun distance (mcarats_ng.init_src), so the
        # sunlight is NOT weighted with the slit function as a solar job's is; `toa` is the solar route's
        factors = np.zeros((Nz, mca_obj.Ng), dtype=np.float32)
        for ig in range(mca_obj.Ng):
            factors[:, ig] = np.float32(weight[ig]*1.0e-3)
        toa = np.sum(cal_sol_fac(mca_obj.date)*abs_obj.coef['solar']['data']*weight) if source == 'solar+thermal' else 0.0
        return factors, toa
    zz = np.arange(Nz)
    if Nz > 1:
        zz[-1] = zz[-2]
    sol_fac = cal_sol_fac(mca_obj.date)
    solar  = abs_obj.coef['solar']['data']
    slit   = abs_obj.coef['slit_func']['data']
    factors = np.zeros((Nz, mca_obj.Ng), dtype=np.float32)
    for iz in range(Nz):
        norm = np.float32(sol_fac/(weight*slit[zz[iz], :]).sum())
        for ig in range(mca_obj.Ng):
            factors[iz, ig] = norm*solar[ig]*weight[ig]*slit[zz[iz], ig]
    toa = np.sum(sol_fac*solar*weight)
    return factors, toa


def _accumulate(mca_obj, abs_obj, nvar, squeeze):

    """sum over g of factor * variable for every run: list of nvar arrays (dims..., Nrun), plus dims_info and toa"""

    fused = getattr(mca_obj, 'fused', None)
    if fused is not None:
        return _from_fused(fused, nvar, squeeze)

    out0 = mca_out_raw(mca_obj.fnames_out[0][0])
    dims_info = list(out0.data[0]['dims_info'])
    dims = list(out0.data[0]['dims'])
    Nz = dims[dims_info.index('Nz')]
    if nvar in (1, 2) and Nz > 1 and getattr(mca_obj, 'Nview', 1) > 1:
        # (a radiance file of several views -- mcarats_ng with sequences of sensor angles, not in the reference --: its third axis counts
        #  views, not levels; every view is scaled like the reference's one view)
        factors, toa = g_factors(mca_obj, abs_obj, 1)
        factors = np.repeat(factors, Nz, axis=0)
    else:
        factors, toa = g_factors(mca_obj, abs_obj, Nz)

    if squeeze:
        dims_info = [dims_info[i] for i in range(len(dims)) if dims[i] > 1]
        dims = [n for n in dims if n > 1]
    dims_info += ['Nr']
    dims += [mca_obj.Nrun]

    # The same float32 operations in the same order as the reference's loop (sum[..., ir] += raw*factor, g after g), but a run is
    # summed in an array of its own, laid out like the file (Fortran order): element after element in memory instead of every
    # Nrun-th float of a C-ordered array -- the reader of 48 flux files of 13.6 MB took longer than the simulation.
    sums = [np.zeros(dims, dtype=np.float32) for _ in range(nvar)]

    def one_run(ir):
        run = [np.zeros(dims[:-1], dtype=np.float32, order='F') for _ in range(nvar)]
        for ig in range(mca_obj.Ng):
            raw = mca_out_raw(mca_obj.fnames_out[ir][ig])
            fac = factors[:, ig][None, None, :, None]
            for iv in range(nvar):
                scaled = raw.data[iv]['data']*fac
                run[iv] += np.squeeze(scaled) if squeeze else scaled
        for iv in range(nvar):
            sums[iv][..., ir] = run[iv]

    # (the runs side by side, a thread each -- reading and the array operations release the interpreter lock --; inside a run g after g,
    #  as the float32 sum demands.  Reading further ahead or the variables of a file side by side bought nothing: tried)
    if mca_obj.Nrun > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(mca_obj.Nrun, 8)) as pool:
            list(pool.map(one_run, range(mca_obj.Nrun)))
    else:
        one_run(0)
    return sums, dims_info, toa


def _from_fused(fused, nvar, squeeze):

    """per-run fields gathered on the device by `mcarats_ng(abs_obj=...)`, brought to the file route's shapes"""

    if nvar == 2 and 'rdir' not in fused:      # point radiometers of a thermal job: no sun, the run field is the diffuse part and the direct part 0
        runs = np.stack([fused['rad']['runs'], np.zeros_like(fused['rad']['runs'])])
    elif nvar == 2:     # point radiometers: the run field holds diffuse + direct, the direct part is known per run -> (diffuse, direct)
        runs = np.stack([fused['rad']['runs']-fused['rdir']['runs'], fused['rdir']['runs']])
    else:
        runs = fused['flux']['runs'] if nvar == 3 else fused['rad']['runs'][None]      # (nvar, Nz, Ny, Nx, Nr)
    dims_info = ['Nx', 'Ny', 'Nz', 'Nt', 'Nr']
    sums = []
    for iv in range(nvar):
        a = np.transpose(runs[iv], (2, 1, 0, 3))[:, :, :, None, :]                   # (Nx, Ny, Nz, Nt=1, Nr)
        sums.append(a)
    if squeeze:
        keep = [i for i, n in enumerate(sums[0].shape[:-1]) if n > 1] + [4]
        dims_info = [dims_info[i] for i in keep]
        sums = [a.reshape([a.shape[i] for i in keep]) for a in sums]
    return [np.ascontiguousarray(a) for a in sums], dims_info, fused['toa']


def read_flux_mca_out(mca_obj, abs_obj, mode='mean', squeeze=True):

    """
    Fluxes summed over g, per run ('all') or mean and population standard deviation over runs ('mean').
    Output variables of the solver, in order: direct-down, total-down, up (reference: mca_out.py:350-352).
    keys: f_up, f_down, f_down_direct, f_down_diffuse (+ *_std for 'mean'), toa, N_photon, N_run
    """

    mode = mode.lower()
    (f_down_direct, f_down, f_up), dims_info, toa = _accumulate(mca_obj, abs_obj, 3, squeeze)
    fields = [('f_down', f_down, 'Global downwelling flux'), ('f_up', f_up, 'Global upwelling flux'),
              ('f_down_direct', f_down_direct, 'Direct downwelling flux'),
              ('f_down_diffuse', f_down-f_down_direct, 'Diffuse downwelling flux')]

    data = {'toa': {'data': toa, 'name': 'TOA without SZA', 'units': 'W/m^2/nm'}}
    if mode == 'all':
        for key, arr, name in fields:
            data[key] = {'data': arr, 'name': name, 'units': 'W/m^2/nm', 'dims_info': dims_info}
    elif mode == 'mean':
        # (numpy's own reductions, the reference's: eight of them over millions of cells, side by side -- they release the interpreter lock)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=8) as pool:
            means = list(pool.map(lambda f: np.mean(f[1], axis=-1), fields))
            stds = list(pool.map(lambda f: np.std(f[1], axis=-1), fields))
        for (key, arr, name), v in zip(fields, means):
            data[key] = {'data': v, 'name': name+' (mean)', 'units': 'W/m^2/nm', 'dims_info': dims_info[:-1]}
        for (key, arr, name), v in zip(fields, stds):
            data[key+'_std'] = {'data': v, 'name': name+' (standard deviation)', 'units': 'W/m^2/nm', 'dims_info': dims_info[:-1]}
    else:
        raise OSError('Error [read_flux_mca_out]: Do not support <mode=%s>.' % mode)
    data['N_photon'] = {'data': mca_obj.photons, 'name': 'Number of photons', 'units': 'N/A'}
    data['N_run']    = {'data': mca_obj.Nrun, 'name': 'Number of runs', 'units': 'N/A'}
    return data


def read_heating_mca_out(mca_obj, abs_obj, mode='mean', squeeze=True):

    """
    target='heating rate' (er3t/rtm/mca/mcarats.py:279-283: Flx_mflx = 3, Flx_mhrt = 1): the fluxes of `read_flux_mca_out` plus
    `heating_rate` (+ `heating_rate_std`): the fourth variable of every job's output, absorbed power per unit volume on the LAYER
    grid (Nx, Ny, Nz layers), scaled per g like the fluxes (the factor of a layer is that of its lower level: the slit function is
    given per layer, mca_out.py:313-328) and summed over g.  Units: W/m^3/nm; divided by air density x c_p: K/s.
    (The reference's reader has no such branch, er3t/rtm/mca/mca_out.py:202-205: its `mca_out_ng` ends without data for this target.)
    Thermal object (mcarats_ng(source='thermal'), Flx_mhrt = 2): the variable is the NET absorbed power per unit volume, absorbed - emitted
    (negative: longwave cooling), combined with the thermal g-sum: sum_g weight[ig] x_g / 1000, no solar spectrum, no slit function.
    Solar+thermal object (source='solar+thermal'): the same variable and the same g-sum, the absorbed sunlight included.
    """

    data = read_flux_mca_out(mca_obj, abs_obj, mode=mode, squeeze=squeeze)
    out0 = mca_out_raw(mca_obj.fnames_out[0][0])
    if len(out0.data) < 4:
        raise OSError('Error [read_heating_mca_out]: <%s> holds no heating-rate variable.' % mca_obj.fnames_out[0][0])
    dims = list(out0.data[3]['dims']); dims_info = list(out0.data[3]['dims_info'])
    nlay = dims[dims_info.index('Nz')]
    factors, _ = g_factors(mca_obj, abs_obj, nlay+1)
    if squeeze:
        dims_info = [dims_info[i] for i in range(len(dims)) if dims[i] > 1]
        dims = [n for n in dims if n > 1]
    hr = np.zeros(dims+[mca_obj.Nrun], dtype=np.float32)
    for ir in range(mca_obj.Nrun):
        run = np.zeros(dims, dtype=np.float32, order='F')
        for ig in range(mca_obj.Ng):
            scaled = mca_out_raw(mca_obj.fnames_out[ir][ig]).data[3]['data']*factors[:nlay, ig][None, None, :, None]
            run += np.squeeze(scaled) if squeeze else scaled
        hr[..., ir] = run
    dims_info = dims_info+['Nr']
    # (the same variable under both estimators of the tally, mcarats_ng's <heating_estimator>: the default's names are what they were)
    est = ', path-length estimator' if getattr(mca_obj, 'heating_estimator', 'collision') == 'path' else ''
    what = 'Net absorbed power per unit volume' if getattr(mca_obj, 'source', 'solar') in ('thermal', 'solar+thermal') else 'Absorbed power per unit volume'
    if mode.lower() == 'all':
        data['heating_rate'] = {'data': hr, 'name': what+est, 'units': 'W/m^3/nm', 'dims_info': dims_info}
    else:
        data['heating_rate'] = {'data': np.mean(hr, axis=-1), 'name': '%s (mean%s)' % (what, est), 'units': 'W/m^3/nm', 'dims_info': dims_info[:-1]}
        data['heating_rate_std'] = {'data': np.std(hr, axis=-1), 'name': '%s (standard deviation%s)' % (what, est), 'units': 'W/m^3/nm', 'dims_info': dims_info[:-1]}
    return data


def read_radiance_mca_out(mca_obj, abs_obj, mode='mean', squeeze=True):

    """
    Radiance summed over g, per run ('all') or mean and population standard deviation over runs ('mean').
    keys: rad (+ rad_std for 'mean'), toa, N_photon, N_run      (reference: mca_out.py:412-505)
    Thermal and solar+thermal objects add `bt`, the brightness temperature of the g-combined radiance at the band centre.  Solar+thermal:
    the g-sum is the thermal route's, sum_g weight[ig] x_g / 1000 with NO slit function (every job is absolute already: its Src_fsol holds
    the solar spectrum); `toa` is the solar route's; `bt` includes the reflected sunlight, as a 3.9 um channel measures it.
    """

    mode = mode.lower()
    (rad,), dims_info, toa = _accumulate(mca_obj, abs_obj, 1, squeeze)

    data = {'toa': {'data': toa, 'name': 'TOA without SZA', 'units': 'W/m^2/nm'}}
    if mode == 'all':
        data['rad'] = {'data': rad, 'name': 'Radiance', 'units': 'W/m^2/nm/sr', 'dims_info': dims_info}
    elif mode == 'mean':
        data['rad']     = {'data': np.mean(rad, axis=-1), 'name': 'Radiance (mean)', 'units': 'W/m^2/nm/sr', 'dims_info': dims_info[:-1]}
        data['rad_std'] = {'data': np.std(rad, axis=-1), 'name': 'Radiance (standard deviation)', 'units': 'W/m^2/nm/sr', 'dims_info': dims_info[:-1]}
    else:
        raise OSError('Error [read_radiance_mca_out]: Do not support <mode=%s>.' % mode)
    source = getattr(mca_obj, 'source', 'solar')
    if source in ('thermal', 'solar+thermal'):
        # brightness temperature of the g-combined radiance at the band centre (W m-2 sr-1 nm-1 -> um-1)
        from er3t_amd.thermal import brightness_temperature
        if source == 'thermal':
            data['toa']['name'] = 'TOA without SZA (none: thermal source)'
        data['bt'] = {'data': brightness_temperature(mca_obj.wlen_um, data['rad']['data'].astype(np.float64)*1.0e3).astype(np.float32),
                      'name': 'Brightness temperature' + (', reflected sunlight included' if source == 'solar+thermal' else '')
                              + (' (of the mean radiance)' if mode == 'mean' else ''), 'units': 'K',
                      'dims_info': data['rad']['dims_info']}
    if getattr(mca_obj, 'pixel_errors', False):
        se, se_info = read_pixel_errors(mca_obj, abs_obj, mode=mode, squeeze=squeeze)
        what = 'per run' if mode == 'all' else 'of the mean over runs'
        data['rad_se'] = {'data': se, 'name': 'Radiance (standard error %s, from the histories)' % what, 'units': 'W/m^2/nm/sr', 'dims_info': se_info}
        if 'bt' in data:
            # the error of the brightness temperature to first order: rad_se / (dB/dT at bt), the radiance per um as bt takes it
            from er3t_amd.thermal import dplanck_dT
            with np.errstate(divide='ignore', invalid='ignore'):
                d = dplanck_dT(mca_obj.wlen_um, data['bt']['data'].astype(np.float64))
                bt_se = np.where(d > 0.0, se.astype(np.float64)*1.0e3/d, 0.0).astype(np.float32)
            data['bt_se'] = {'data': bt_se, 'name': 'Brightness temperature (standard error %s, from the histories)' % what, 'units': 'K',
                             'dims_info': se_info}
    data['N_photon'] = {'data': mca_obj.photons, 'name': 'Number of photons', 'units': 'N/A'}
    data['N_run']    = {'data': mca_obj.Nrun, 'name': 'Number of runs', 'units': 'N/A'}
    return data


def pixel_error_runs(se_jobs, factors):

    """
    The g combination of the per-pixel standard errors (mcarats_ng(pixel_errors=True), Rad_mserr = 1).  Jobs of different g and of different
    runs have different seeds and are independent, so variances add: per run  rad_se_run^2 = sum_g factor[view, g]^2 se_g^2,  with the
    float32 factors of `rad` (g_factors).  se_jobs: (Nrun, Ng, nview, nyr, nxr), factors: (nview, Ng).  Returns the VARIANCES, float64
    (Nrun, nview, nyr, nxr), summed g after g.
    """

    se = np.asarray(se_jobs, dtype=np.float64)
    f = np.asarray(factors, dtype=np.float64)
    var = np.zeros((se.shape[0],)+se.shape[2:], dtype=np.float64)
    for ig in range(se.shape[1]):
        t = f[:, ig][None, :, None, None]*se[:, ig]
        var += t*t
    return var


def read_pixel_errors(mca_obj, abs_obj, mode='mean', squeeze=True):

    """
    rad_se of mcarats_ng(pixel_errors=True): the standard error of `rad` from the histories themselves, in the layout of `rad`
    (Nx, Ny, Nview; axes of length 1 dropped with squeeze).  'all': per run (a last axis Nr), sqrt(sum_g f_g^2 se_g^2); 'mean': of the mean
    over runs, sqrt(sum_r rad_se_r^2) / Nrun.  The file route reads the jobs' .err.bin files; the fused route has kept the same arrays
    (mcarats_ng.run_fused).  Returns (array float32, dims_info).
    """

    from er3t_amd.rtm.mca.mca_inp import mca_inp_read
    from er3t_amd.rtm.mca.mca_exe import errors_fname, read_errors
    mode = mode.lower()
    if mode not in ('mean', 'all'):
        raise OSError('Error [read_pixel_errors]: Do not support <mode=%s>.' % mode)
    fused = getattr(mca_obj, 'fused', None)
    if fused is not None and 'se' in fused:
        se_jobs = fused['se']
    else:
        g9 = _weights_geometry(mca_inp_read(mca_obj.fnames_inp[0][0]))
        se_jobs = np.stack([np.stack([read_errors(errors_fname(mca_obj.fnames_out[ir][ig]), g9[0], g9[1], g9[2]) for ig in range(mca_obj.Ng)])
                            for ir in range(mca_obj.Nrun)])
    factors, _ = g_factors(mca_obj, abs_obj, 1)
    var = pixel_error_runs(se_jobs, np.repeat(factors, se_jobs.shape[2], axis=0))      # (every view scaled like the one view of `rad`)
    if mode == 'all':
        a = np.transpose(np.sqrt(var), (3, 2, 1, 0))                                    # (Nx, Ny, Nview, Nr)
        info = ['Nx', 'Ny', 'Nz', 'Nr']
        keep = [i for i in range(3) if a.shape[i] > 1 or not squeeze]+[3]
    else:
        a = np.transpose(np.sqrt(var.sum(axis=0))/var.shape[0], (2, 1, 0))              # (Nx, Ny, Nview)
        info = ['Nx', 'Ny', 'Nz']
        keep = [i for i in range(3) if a.shape[i] > 1 or not squeeze]
    if not squeeze:                                                                     # (the file route's Nt axis)
        a = a[:, :, :, None]
        info = info[:3]+['Nt']+info[3:]
        keep = list(range(a.ndim))
    a = a.reshape([a.shape[i] for i in keep])
    return np.ascontiguousarray(a.astype(np.float32)), [info[i] for i in keep]


def read_radiometer_mca_out(mca_obj, abs_obj, mode='mean', squeeze=True):

    """
    sensor_type 'irradiance' | 'actinic' (point radiometers, one pixel over the hemisphere around the sensor's axis): per sensor
    (the view axis), summed over g, per run ('all') or mean and population standard deviation over runs ('mean').
    keys: f, f_diffuse, f_direct (+ *_std for 'mean'), toa, N_photon, N_run.  The files hold the cosine-weighted (irradiance) or
    plain (actinic) mean radiance over the hemisphere: scattered light as `rad`, the direct sun as `rdir`; the fluxes are pi (irradiance)
    or 2 pi (actinic flux) times them.  Thermal object (mcarats_ng(source='thermal'): a pyrgeometer, an IR radiometer): the thermal g-sum,
    sum_g weight[ig] x_g / 1000 with no solar spectrum and no slit function; `rdir` is 0 -- a thermal job has no sun --, so f_direct = 0
    and f = f_diffuse.
    """

    mode = mode.lower()
    (rad, rdir), dims_info, toa = _accumulate(mca_obj, abs_obj, 2, squeeze)
    solid = np.float32(np.pi if str(mca_obj.sensor_type).lower() == 'irradiance' else 2.0*np.pi)
    f_diffuse, f_direct = rad*solid, rdir*solid
    fields = [('f', f_diffuse+f_direct, 'Total'), ('f_diffuse', f_diffuse, 'Diffuse'), ('f_direct', f_direct, 'Direct')]
    what = 'irradiance' if str(mca_obj.sensor_type).lower() == 'irradiance' else 'actinic flux'
    data = {'toa': {'data': toa, 'name': 'TOA without SZA' + (' (none: thermal source)' if getattr(mca_obj, 'source', 'solar') == 'thermal' else ''),
                    'units': 'W/m^2/nm'}}
    for key, arr, name in fields:
        if mode == 'all':
            data[key] = {'data': arr, 'name': '%s %s' % (name, what), 'units': 'W/m^2/nm', 'dims_info': dims_info}
        elif mode == 'mean':
            data[key] = {'data': np.mean(arr, axis=-1), 'name': '%s %s (mean)' % (name, what), 'units': 'W/m^2/nm', 'dims_info': dims_info[:-1]}
            data[key+'_std'] = {'data': np.std(arr, axis=-1), 'name': '%s %s (standard deviation)' % (name, what), 'units': 'W/m^2/nm',
                                'dims_info': dims_info[:-1]}
        else:
            raise OSError('Error [read_radiometer_mca_out]: Do not support <mode=%s>.' % mode)
    if getattr(mca_obj, 'pixel_errors', False):
        # (a thermal job: no direct part, f = f_diffuse = solid angle x rad, and so is its error)
        se, se_info = read_pixel_errors(mca_obj, abs_obj, mode=mode, squeeze=squeeze)
        data['rad_se'] = {'data': se, 'name': 'Mean radiance over the hemisphere (standard error, from the histories)', 'units': 'W/m^2/nm/sr', 'dims_info': se_info}
        data['f_se'] = {'data': se*solid, 'name': 'Total %s (standard error, from the histories)' % what, 'units': 'W/m^2/nm', 'dims_info': se_info}
    data['N_photon'] = {'data': mca_obj.photons, 'name': 'Number of photons', 'units': 'N/A'}
    data['N_run']    = {'data': mca_obj.Nrun, 'name': 'Number of runs', 'units': 'N/A'}
    return data


class weights_reducer:

    """
    The g / run reduction of the per-cell emission weights (mcarats_ng(emission_weights=True), Rad_mwgt = 1), with the factors of `rad`:
    per run sum_g factor[ig] * K_g, over runs the mean and the population standard deviation.  Fed JOB BY JOB (add, then end_run after the
    last g of a run) and summed in float64 as it goes: the arrays can be gigabytes, so what it holds does not grow with the number of
    jobs -- the current run, the sum and the sum of squares over runs, and, only with keep_runs, one array per run (mode 'all').
    `planck` is taken once, from the first job.  jobs_fed counts the calls of add.
    """

    def __init__(self, factors, keep_runs=False):
        self.factors = np.asarray(factors, dtype=np.float64).ravel()
        self.keep_runs = keep_runs
        self.run = self.s1 = self.s2 = self.planck = None
        self.runs, self.nrun, self.jobs_fed = [], 0, 0

    def add(self, ig, weights, planck=None):
        if self.run is None:
            self.run = np.zeros(np.shape(weights), dtype=np.float64)
            self.s1, self.s2 = np.zeros_like(self.run), np.zeros_like(self.run)
        if self.planck is None and planck is not None:
            self.planck = np.array(planck, dtype=np.float32)
        self.run += self.factors[ig]*np.asarray(weights, dtype=np.float64)
        self.jobs_fed += 1

    def end_run(self):
        self.s1 += self.run
        self.s2 += self.run*self.run
        if self.keep_runs:
            self.runs.append(self.run.astype(np.float32))
        self.run[...] = 0.0
        self.nrun += 1

    def mean(self):
        return (self.s1/self.nrun).astype(np.float32)

    def std(self):
        m = self.s1/self.nrun
        return np.sqrt(np.maximum(self.s2/self.nrun-m*m, 0.0)).astype(np.float32)


def _weights_geometry(nml):
    """(nview, nyr, nxr, nz3, ny, nx, nz, nyb, nxb) of a job with <Rad_mwgt=1> from its namelist"""
    g = lambda k, d: int(np.ravel(nml.get(k, d) if nml.get(k) is not None else d)[0])
    sfc2d = bool(nml.get('Sfc_inpfile')) and g('Sfc_nxb', 0) > 0
    return (g('Rad_nrad', 1), g('Rad_nyr', 1), g('Rad_nxr', 1), g('Atm_nz3', 0), g('Atm_ny', 1), g('Atm_nx', 1), g('Atm_nz', 1),
            g('Sfc_nyb', 1) if sfc2d else 1, g('Sfc_nxb', 1) if sfc2d else 1)


def _weights_fields(k, geom, squeeze, pixels=True):
    """K (npix, ncell[, Nr]) or planck (ncell,) in tally order -> its three parts in the layout of the 3-D outputs (f_up, heating_rate), the pixel
    axes (Nxr, Nyr, Nview) last: voxels (Nx, Ny, Nz3, ...), layers (Nz, ...), surface (Nxb, Nyb, ...).  squeeze drops pixel axes of length 1"""
    nview, nyr, nxr, nz3, ny, nx, nz, nyb, nxb = geom
    nvox = nx*ny*nz3
    k = np.asarray(k)
    if not pixels:
        return {'': np.ascontiguousarray(np.transpose(k[:nvox].reshape(nz3, ny, nx), (2, 1, 0))), '_layers': np.ascontiguousarray(k[nvox:nvox+nz]),
                '_surface': np.ascontiguousarray(np.transpose(k[nvox+nz:].reshape(nyb, nxb), (1, 0)))}
    tail = k.shape[2:]
    pix = (nview, nyr, nxr)
    v = k[:, :nvox].reshape(pix+(nz3, ny, nx)+tail)
    l = k[:, nvox:nvox+nz].reshape(pix+(nz,)+tail)
    s = k[:, nvox+nz:].reshape(pix+(nyb, nxb)+tail)
    nt = len(tail)
    v = np.transpose(v, (5, 4, 3, 2, 1, 0)+tuple(range(6, 6+nt)))
    l = np.transpose(l, (3, 2, 1, 0)+tuple(range(4, 4+nt)))
    s = np.transpose(s, (4, 3, 2, 1, 0)+tuple(range(5, 5+nt)))
    if squeeze:
        def drop(a, first):
            keep = [i for i, n in enumerate(a.shape) if i < first or i >= first+3 or n > 1]
            return a.reshape([a.shape[i] for i in keep])
        v, l, s = drop(v, 3), drop(l, 1), drop(s, 2)
    return {'': np.ascontiguousarray(v), '_layers': np.ascontiguousarray(l), '_surface': np.ascontiguousarray(s)}


def read_emission_weights(mca_obj, abs_obj, mode='mean', squeeze=True):

    """
    The per-cell emission weights of mcarats_ng(camera_method='backward', emission_weights=True): K[pixel][cell], the share of a pixel's
    reading that comes from a cell per unit Planck radiance there, combined over g and runs with the factors of `rad` (sum_g weight[ig] x_g
    / 1000; mean and standard deviation over runs), so that  rad = sum over all cells of emission_weight * emission_planck  (jobs of
    mcarats_ng carry Src_flx = 1).  keys: emission_weight (Nx, Ny, Nz3, pixels...), emission_weight_layers (Nz, pixels...),
    emission_weight_surface (Nxb, Nyb, pixels...) -- pixel axes (Nxr, Nyr, Nview), those of length 1 dropped with squeeze; 'all' adds Nr --
    (+ *_std for 'mean') and, once, emission_planck, emission_planck_layers, emission_planck_surface [W m-2 sr-1 um-1].  The file route reads
    the jobs' .wgt.bin files one at a time; the fused route has reduced the same arrays while the jobs ran (mcarats_ng.run_fused).
    """

    from er3t_amd.rtm.mca.mca_inp import mca_inp_read
    from er3t_amd.rtm.mca.mca_exe import weights_fname
    mode = mode.lower()
    if mode not in ('mean', 'all'):
        raise OSError('Error [read_emission_weights]: Do not support <mode=%s>.' % mode)
    geom = _weights_geometry(mca_inp_read(mca_obj.fnames_inp[0][0]))
    fused = getattr(mca_obj, 'fused', None)
    if fused is not None and 'wgt' in fused:
        red = fused['wgt']
    else:
        factors, _ = g_factors(mca_obj, abs_obj, 1)
        red = weights_reducer(factors[0], keep_runs=(mode == 'all'))
        npix = geom[0]*geom[1]*geom[2]
        for ir in range(mca_obj.Nrun):
            for ig in range(mca_obj.Ng):
                raw = np.fromfile(weights_fname(mca_obj.fnames_out[ir][ig]), dtype='<f4')
                ncell = raw.size//(npix+1)
                if raw.size != (npix+1)*ncell:
                    raise OSError('Error [read_emission_weights]: <%s> does not hold %d + 1 rows.' % (weights_fname(mca_obj.fnames_out[ir][ig]), npix))
                red.add(ig, raw[:npix*ncell].reshape(npix, ncell), raw[npix*ncell:])
                del raw
            red.end_run()
    data = {}
    info = {'': ['Nx', 'Ny', 'Nz3'], '_layers': ['Nz'], '_surface': ['Nxb', 'Nyb']}
    def put(key, fields, name, units, extra):
        for suf, arr in fields.items():
            data[key+suf] = {'data': arr, 'name': name, 'units': units, 'dims_info': info[suf]+extra}
    pixdims = [d for d, n in zip(['Nxr', 'Nyr', 'Nview'], (geom[2], geom[1], geom[0])) if n > 1 or not squeeze]
    if mode == 'all':
        if not red.runs:
            raise OSError('Error [read_emission_weights]: the runs were not kept; use <mode=\'mean\'>.')
        put('emission_weight', _weights_fields(np.stack(red.runs, axis=-1), geom, squeeze), 'Emission weight', 'N/A (per nm: the g-sum of rad)', pixdims+['Nr'])
    else:
        put('emission_weight', _weights_fields(red.mean(), geom, squeeze), 'Emission weight (mean)', 'N/A (per nm: the g-sum of rad)', pixdims)
        put('emission_weight_std', _weights_fields(red.std(), geom, squeeze), 'Emission weight (standard deviation)', 'N/A (per nm: the g-sum of rad)', pixdims)
    put('emission_planck', _weights_fields(red.planck, geom, squeeze, pixels=False), 'Planck radiance of the cells', 'W/m^2/um/sr', [])
    return data


def _profile_fields(p, geom, squeeze):
    """(2, npix, nz+1[, Nr]) in tally order -> (weight, contribution), each (Nxr, Nyr, Nview, Nz+1[, Nr]); squeeze drops pixel axes of length 1"""
    nview, nyr, nxr, nrow = geom
    p = np.asarray(p)
    tail = p.shape[3:]
    a = np.transpose(p.reshape((2, nview, nyr, nxr, nrow)+tail), (0, 3, 2, 1, 4)+tuple(range(5, 5+len(tail))))
    if squeeze:
        a = a.reshape([n for i, n in enumerate(a.shape) if not (1 <= i <= 3) or n > 1])
    return np.ascontiguousarray(a[0]), np.ascontiguousarray(a[1])


def read_view_profiles(mca_obj, abs_obj, mode='mean', squeeze=True):

    """
    The per-layer profiles of mcarats_ng(view_method='backward', view_profiles=True): for every pixel the vertical weighting function
    view_weight[..., k] -- the share of the pixel's radiance that comes from layer k (k = 0 ... Nz-1 from the surface up; a layer of the 3-D
    region: all its voxels) or from the surface (k = Nz) per unit Planck radiance there -- and view_contribution[..., k], that share itself,
    both combined over g and runs with the factors of `rad` (sum_g weight[ig] x_g / 1000; mean and standard deviation over runs), so that
    rad = view_contribution.sum(-1)  (jobs of mcarats_ng carry Src_flx = 1).  Axes: (Nxr, Nyr, Nview), those of length 1 dropped with
    squeeze, then Nz+1; 'all' adds Nr.  keys: view_weight, view_contribution (+ *_std for 'mean') and view_layer_planck =
    view_contribution / view_weight [W m-2 sr-1 um-1], the layer's effective Planck radiance as the pixel sees it, NaN where the weight is 0.
    The file route reads the jobs' .prf.bin files one at a time; the fused route has reduced the same arrays while the jobs ran.
    """

    from er3t_amd.rtm.mca.mca_inp import mca_inp_read
    from er3t_amd.rtm.mca.mca_exe import profiles_fname, read_profiles
    mode = mode.lower()
    if mode not in ('mean', 'all'):
        raise OSError('Error [read_view_profiles]: Do not support <mode=%s>.' % mode)
    g9 = _weights_geometry(mca_inp_read(mca_obj.fnames_inp[0][0]))
    geom = (g9[0], g9[1], g9[2], g9[6]+1)
    fused = getattr(mca_obj, 'fused', None)
    if fused is not None and 'prf' in fused:
        red = fused['prf']
    else:
        factors, _ = g_factors(mca_obj, abs_obj, 1)
        red = weights_reducer(factors[0], keep_runs=(mode == 'all'))
        for ir in range(mca_obj.Nrun):
            for ig in range(mca_obj.Ng):
                red.add(ig, read_profiles(profiles_fname(mca_obj.fnames_out[ir][ig]), geom[0]*geom[1]*geom[2], geom[3]))
            red.end_run()
    pixdims = [d for d, n in zip(['Nxr', 'Nyr', 'Nview'], (geom[2], geom[1], geom[0])) if n > 1 or not squeeze]+['Nz+1']
    units = 'N/A (per nm: the g-sum of rad)'
    data = {}
    if mode == 'all':
        if not red.runs:
            raise OSError('Error [read_view_profiles]: the runs were not kept; use <mode=\'mean\'>.')
        k, c = _profile_fields(np.stack(red.runs, axis=-1), geom, squeeze)
        data['view_weight'] = {'data': k, 'name': 'Weighting function of the view', 'units': units, 'dims_info': pixdims+['Nr']}
        data['view_contribution'] = {'data': c, 'name': 'Contribution to the radiance', 'units': 'W/m^2/nm/sr', 'dims_info': pixdims+['Nr']}
    else:
        k, c = _profile_fields(red.mean(), geom, squeeze)
        ks, cs = _profile_fields(red.std(), geom, squeeze)
        data['view_weight'] = {'data': k, 'name': 'Weighting function of the view (mean)', 'units': units, 'dims_info': pixdims}
        data['view_weight_std'] = {'data': ks, 'name': 'Weighting function of the view (standard deviation)', 'units': units, 'dims_info': pixdims}
        data['view_contribution'] = {'data': c, 'name': 'Contribution to the radiance (mean)', 'units': 'W/m^2/nm/sr', 'dims_info': pixdims}
        data['view_contribution_std'] = {'data': cs, 'name': 'Contribution to the radiance (standard deviation)', 'units': 'W/m^2/nm/sr', 'dims_info': pixdims}
    with np.errstate(divide='ignore', invalid='ignore'):
        b = np.where(k != 0.0, c.astype(np.float64)/k.astype(np.float64), np.nan).astype(np.float32)
    data['view_layer_planck'] = {'data': b, 'name': 'Effective Planck radiance of the layers as the pixels see them', 'units': 'W/m^2/um/sr',
                                 'dims_info': list(data['view_weight']['dims_info'])}
    return data


class mca_out_ng:

    """
    Collect the results of a `mcarats_ng` simulation.

    Input:
        fname=    : result cache to write/read (HDF5 when h5py is installed and the name ends in .h5/.hdf5, else .npz)
        mca_obj=  : the mcarats_ng object;   abs_obj=: the absorption object (coef['weight'|'solar'|'slit_func'])
        mode=     : 'mean' | 'all';   squeeze=: drop axes of length 1;   overwrite=: recompute even if <fname> exists

    Output:
        self.data[key]['data'|'name'|'units'|'dims_info'], keys as returned by read_flux_mca_out / read_radiance_mca_out

    Same three call shapes as the reference (er3t/rtm/mca/mca_out.py:160-177): cache only, objects + cache, objects only.
    """

    def __init__(self, fname=None, mca_obj=None, abs_obj=None, mode='mean', overwrite=False, squeeze=True,
                 quiet=False, verbose=False):

        self.mode      = mode
        self.quiet     = quiet
        self.verbose   = verbose
        self.overwrite = overwrite
        self.squeeze   = squeeze
        self.fname     = fname
        self.mca       = mca_obj
        self.abs       = abs_obj

        have_objs = (mca_obj is not None) and (abs_obj is not None)
        if (fname is not None) and os.path.exists(fname) and (not overwrite):
            self.load()
        elif have_objs and (fname is not None):
            self.run()
            self.dump()
        elif have_objs:
            self.run()
        else:
            raise OSError('Error [mca_out_ng]: Please provide both <mca_obj> and <abs_obj> to proceed.')

    def run(self):
        if self.verbose:
            print('Message [mca_out_ng]: Reading <%s> ...' % self.mca.target.lower())
        if self.mca.target in ['flux', 'flux0']:
            self.data = read_flux_mca_out(self.mca, self.abs, mode=self.mode, squeeze=self.squeeze)
        elif self.mca.target == 'radiance' and str(getattr(self.mca, 'sensor_type', '')).lower() in ('irradiance', 'actinic'):
            self.data = read_radiometer_mca_out(self.mca, self.abs, mode=self.mode, squeeze=self.squeeze)
        elif self.mca.target == 'radiance':
            self.data = read_radiance_mca_out(self.mca, self.abs, mode=self.mode, squeeze=self.squeeze)
        elif self.mca.target == 'heating rate':
            self.data = read_heating_mca_out(self.mca, self.abs, mode=self.mode, squeeze=self.squeeze)
        else:
            raise OSError('Error [mca_out_ng]: Cannot read results of <target=%s>.' % self.mca.target)
        if getattr(self.mca, 'emission_weights', False):
            self.data.update(read_emission_weights(self.mca, self.abs, mode=self.mode, squeeze=self.squeeze))
        if getattr(self.mca, 'view_profiles', False):
            self.data.update(read_view_profiles(self.mca, self.abs, mode=self.mode, squeeze=self.squeeze))

    # ---- result cache ------------------------------------------------------------------------
    @staticmethod
    def _is_hdf5(fname):
        return fname.lower().endswith(('.h5', '.hdf5', '.hdf'))

    def dump(self):
        if not self.quiet:
            print('Message [mca_out_ng]: Saving <%s> into <%s> ...' % (self.mca.target.lower(), self.fname))
        mode = self.mode.lower()
        if self._is_hdf5(self.fname):
            try:
                import h5py
            except ImportError:
                raise OSError('Error [mca_out_ng]: <%s> needs the h5py package; use a .npz file name instead.' % self.fname)
            with h5py.File(self.fname, 'w') as f:
                g = f.create_group(mode)
                for key, item in self.data.items():
                    if isinstance(item['data'], np.ndarray):
                        g.create_dataset(key, data=item['data'], compression='gzip', compression_opts=9, chunks=True)
                    else:
                        g[key] = item['data']
                    for k0, v0 in item.items():
                        if k0 != 'data':
                            g[key].attrs[k0] = np.bytes_(str(v0)) if k0 == 'dims_info' else v0
        else:
            flat = {}
            for key, item in self.data.items():
                for k0, v0 in item.items():
                    flat['%s/%s/%s' % (mode, key, k0)] = np.asarray(v0)
            with open(self.fname, 'wb') as f:
                np.savez_compressed(f, **flat)

    def load(self):
        if self.verbose:
            print('Message [mca_out_ng]: Reading from <%s> ...' % self.fname)
        self.data = {}
        if self._is_hdf5(self.fname):
            try:
                import h5py
            except ImportError:
                raise OSError('Error [mca_out_ng]: <%s> needs the h5py package.' % self.fname)
            with h5py.File(self.fname, 'r') as f:
                g = f[self.mode]
                for key in g.keys():
                    self.data[key] = {'data': g[key][...]}
                    for k0, v0 in g[key].attrs.items():
                        self.data[key][k0] = v0
        else:
            with np.load(self.fname, allow_pickle=False) as z:
                for full in z.files:
                    mode, key, k0 = full.split('/')
                    if mode != self.mode:
                        continue
                    v = z[full]
                    self.data.setdefault(key, {})[k0] = v if k0 == 'data' else (list(v) if v.ndim > 0 else v.item())
