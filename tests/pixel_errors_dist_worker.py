"""
Worker of tests/test_gpu_pixel_errors.py::test_two_ranks_match_one: one process per rank under torch.distributed.run, backend 'gloo', both
ranks on the ONE GPU of a test box.  A thermal satellite job with two views served backwards with per-pixel standard errors
(view_method='backward', pixel_errors=True: Rad_mvbwd = 1, Rad_mserr = 1) under a synthetic cloud field at 11 um, through the file route --
job by job, every rank its shard of [0, N), the raw sums of the scores and of their squares all-reduced before the read-out, rank 0 writing
out.bin and .err.bin -- and through the fused route under the same seeds.  Rank 0 then runs the same jobs again alone.  The same histories,
so the same raw sums up to their order.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P tests/pixel_errors_dist_worker.py <outdir>
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(outdir):
    import torch
    import torch.distributed as dist
    dist.init_process_group('gloo')
    rank = dist.get_rank()

    import er3t_amd.rtm.mca as mca
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from er3t_amd.rtm.mca.mca_exe import JobRunner, run_job, get_runner, errors_fname, read_errors
    from er3t_amd.rtm.mca.mca_out import g_factors, pixel_error_runs
    from tests.golden import inputs as gin

    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=2)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(outdir, 'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target='radiance', surface_albedo=0.2, source='thermal', view_method='backward',
              pixel_errors=True, Nrun=1, photons=1e5, weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True,
              date=gin.DATE, quiet=True, sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
    np.random.seed(7)
    m = mca.mcarats_ng(fdir=os.path.join(outdir, 'file'), **kw)
    both = get_runner()
    assert both.world == 2
    kernel = both.sol.kernel_name()
    capped = both.sol.debug_backward_views(1, 0, 0)[3]
    # the tensors of the job run last (r00.g001), all-reduced: the raw sums of the whole job on either rank
    dist_rad_raw, dist_rad2_raw = both._tensors[0][0].cpu().numpy().copy(), both._tensors[0][5].cpu().numpy().copy()
    dist.barrier()
    np.random.seed(7)
    fu = mca.mcarats_ng(fdir=os.path.join(outdir, 'fused'), abs_obj=ab, keep_files=False, **kw)
    dist.barrier()
    if rank == 0:
        ig = 1
        file_se = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data['rad_se']['data']
        fused_se = mca.mca_out_ng(mca_obj=fu, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data['rad_se']['data']
        res = {'kernel': kernel, 'capped': capped, 'dist_rad_raw': dist_rad_raw, 'dist_rad2_raw': dist_rad2_raw,
               'dist_se': read_errors(errors_fname(m.fnames_out[0][ig]), 2, 10, 12), 'dist_file_rad_se': file_se, 'dist_fused_rad_se': fused_se}
        solo = JobRunner(device=0); solo.rank, solo.world = 0, 1
        jobs = [run_job(m.fnames_inp[0][g], os.path.join(outdir, 'solo%d.out.bin' % g), int(m.photons[g]), 0, runner=solo)['se'] for g in range(2)]
        factors, _ = g_factors(m, ab, 1)
        var = pixel_error_runs(np.array([jobs]), np.repeat(factors, 2, axis=0))
        solo_se = np.transpose(np.sqrt(var.sum(axis=0)), (2, 1, 0)).astype(np.float32)
        res.update(solo_se=jobs[ig], solo_file_rad_se=solo_se, solo_fused_rad_se=solo_se)
        # ... and the last job once more into tensors of this test's own: its raw sums from one rank
        nml = mca.mca_inp_read(m.fnames_inp[0][ig])
        solo.load(nml, os.path.dirname(m.fnames_inp[0][ig]), 0)
        rad = torch.zeros(240, dtype=torch.float64, device='cuda:0'); rad2 = torch.zeros(240, dtype=torch.float64, device='cuda:0')
        solo.sol.bind(rad.data_ptr(), None, None, err_ptr=rad2.data_ptr())
        solo.sol.reset(); solo.sol.run(int(m.photons[ig]), seed=int(nml['Wld_jseed'])); solo.sol.sync()
        torch.cuda.synchronize()
        res.update(solo_rad_raw=rad.cpu().numpy().copy(), solo_rad2_raw=rad2.cpu().numpy().copy())
        solo.sol.bind(None, None, None)
        np.savez(os.path.join(outdir, 'result.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
