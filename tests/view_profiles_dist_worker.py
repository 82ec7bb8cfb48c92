"""
Worker of tests/test_gpu_view_profiles.py::test_two_ranks_match_one: one process per rank under torch.distributed.run, backend 'gloo', both
ranks on the ONE GPU of a test box.  A thermal satellite job with two views served backwards with per-layer profiles (view_method='backward',
view_profiles=True: Rad_mvbwd = 1, Rad_mvprf = 1) under a synthetic cloud field at 11 um through the file route: job by job, every rank its
shard of [0, N), the raw image and the raw profiles all-reduced before the read-out and rank 0 writing out.bin and .prf.bin.  Rank 0 then
runs one job file again alone.  The same histories, so the same rows up to the order of the sums.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P tests/view_profiles_dist_worker.py <outdir>
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
    from er3t_amd.rtm.mca.mca_exe import JobRunner, run_job, get_runner, profiles_fname, read_profiles
    from tests.golden import inputs as gin

    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=2)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(outdir, 'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target='radiance', surface_albedo=0.2, source='thermal', view_method='backward',
              view_profiles=True, Nrun=1, photons=1e5, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True,
              date=gin.DATE, quiet=True, sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
    np.random.seed(7)
    m = mca.mcarats_ng(fdir=os.path.join(outdir, 'file'), **kw)
    both = get_runner()
    assert both.world == 2
    kernel = both.sol.kernel_name()
    capped = both.sol.debug_backward_views(1, 0, 0)[3]
    dist.barrier()
    if rank == 0:
        ig = 1
        nphoton = int(m.photons[ig])
        nz = int(mca.mca_inp_read(m.fnames_inp[0][ig])['Atm_nz'])
        raw = mca.mca_out_raw(m.fnames_out[0][ig])
        prf = read_profiles(profiles_fname(m.fnames_out[0][ig]), 2*10*12, nz+1)
        res = {'kernel': kernel, 'capped': capped, 'nz': nz, 'dist_rad': np.transpose(raw.data[0]['data'][:, :, :, 0], (2, 1, 0)),
               'dist_weight': prf[0].reshape(2, 10, 12, nz+1), 'dist_contribution': prf[1].reshape(2, 10, 12, nz+1)}
        solo = JobRunner(device=0); solo.rank, solo.world = 0, 1
        r1 = run_job(m.fnames_inp[0][ig], os.path.join(outdir, 'solo.out.bin'), nphoton, 0, runner=solo)
        res.update(solo_rad=r1['rad'], solo_weight=r1['prf']['weight'], solo_contribution=r1['prf']['contribution'])
        np.savez(os.path.join(outdir, 'result.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
