"""
Worker of tests/test_gpu_emission_weights.py::test_two_ranks_match_one: one process per rank under torch.distributed.run, backend 'gloo',
both ranks on the ONE GPU of a test box (the pattern of tests/backward_dist_worker.py).  Four backward thermal irradiance sensors with
emission weights (camera_method='backward', emission_weights=True: Rad_mbwd = 1, Rad_mwgt = 1) through the file route -- every rank its
shard of [0, N), the bound weights buffer all-reduced with the radiance -- and the fused route; rank 0 then runs one job file again alone:
the same histories, so the same weights up to the order of the sums.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P tests/emission_weights_dist_worker.py <outdir>
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(outdir):
    import torch.distributed as dist
    dist.init_process_group('gloo')
    rank = dist.get_rank()

    import er3t_amd.rtm.mca as mca
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from er3t_amd.rtm.mca.mca_exe import JobRunner, run_job, get_runner, weights_fname, flatten_weights
    from tests.golden import inputs as gin

    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=2)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(outdir, 'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target='radiance', surface_albedo=0.2, source='thermal', camera_method='backward',
              emission_weights=True, Nrun=2, photons=1e5, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True,
              date=gin.DATE, quiet=True, sensor_type='irradiance', sensor_xpos=[0.1, 0.35, 0.6, 0.85], sensor_ypos=0.5,
              sensor_altitude=[10.0, 700.0, 10.0, 5000.0], sensor_zenith_angle=[0.0, 0.0, 20.0, 180.0])
    m = mca.mcarats_ng(fdir=os.path.join(outdir, 'file'), **kw)
    kernel = get_runner().sol.kernel_name()
    capped = get_runner().sol.debug_backward(1, 0, 0)[2]
    mf = mca.mcarats_ng(fdir=os.path.join(outdir, 'fused'), abs_obj=ab, keep_files=False, **kw)
    outf = mca.mca_out_ng(mca_obj=mf, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data if rank == 0 else None
    if rank == 0:
        out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
        res = {'kernel': kernel, 'capped': capped}
        for tag, d in (('file', out), ('fused', outf)):
            res[tag+'_f'] = d['f']['data']
            for s in ('', '_layers', '_surface'):
                res[tag+'_weight'+s] = d['emission_weight'+s]['data']; res[tag+'_planck'+s] = d['emission_planck'+s]['data']
        solo = JobRunner(device=0); solo.rank, solo.world = 0, 1
        ir, ig = 1, 1
        r = run_job(m.fnames_inp[ir][ig], os.path.join(outdir, 'solo.out.bin'), int(m.photons[ir*m.Ng+ig]), 0, runner=solo)
        k, b = flatten_weights(r['wgt'])
        raw = np.fromfile(weights_fname(m.fnames_out[ir][ig]), dtype='<f4')
        res['job_solo_wgt'] = k; res['job_dist_wgt'] = raw[:k.size].reshape(k.shape)
        res['job_solo_planck'] = b; res['job_dist_planck'] = raw[k.size:]
        res['job_solo_rad'] = r['rad'][:, 0, 0]
        np.savez(os.path.join(outdir, 'result.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
