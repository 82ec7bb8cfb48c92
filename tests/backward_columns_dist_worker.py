"""
Worker of tests/test_gpu_backward_columns.py::test_two_ranks_match_one: one process per rank under torch.distributed.run, backend 'gloo', both
ranks on the ONE GPU of a test box.  A thermal satellite job with two views served backwards under independent columns (view_method='backward',
view_columns=True, solver='IPA': Rad_mvbwd = 1, Rad_mvcol = 1) under a synthetic cloud field at 11 um through the file route (job by job, every rank its shard of [0, N)) and the fused route, both under the SAME
job seeds (a clock that stands still and a seeded shuffle, as tests/conftest.py gives the tests of the parent process); rank 0 then runs
one job file again alone.  Everywhere the same histories, so the same image up to the order of the sums.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P tests/backward_columns_dist_worker.py <outdir>
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

    import time as _time
    import er3t_amd.rtm.mca as mca
    import er3t_amd.rtm.mca.mcarats as _m

    class _StillClock:                       # (mcarats_ng seeds its jobs from the clock and shuffles them over the jobs)
        def __getattr__(self, name):
            return getattr(_time, name)

        @staticmethod
        def time():
            return 1759536000.0
    _m.time = _StillClock()
    from er3t_amd.synth import atm_synth, abs_synth, cld_synth
    from er3t_amd.rtm.mca.mca_exe import JobRunner, run_job, get_runner
    from tests.golden import inputs as gin

    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=2)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(outdir, 'atm3d.bin'), quiet=True)
    kw = dict(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target='radiance', surface_albedo=0.2, source='thermal', view_method='backward', view_columns=True, Nrun=2,
              photons=1e5, weights=ab.coef['weight']['data'], solver='IPA', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True,
              sensor_zenith_angle=[0.0, 40.0], sensor_azimuth_angle=[0.0, 70.0])
    np.random.seed(7)
    m = mca.mcarats_ng(fdir=os.path.join(outdir, 'file'), **kw)
    out = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    kernel = get_runner().sol.kernel_name()
    capped = get_runner().sol.debug_backward_views(1, 0, 0)[3]
    np.random.seed(7)
    mf = mca.mcarats_ng(fdir=os.path.join(outdir, 'fused'), abs_obj=ab, keep_files=False, **kw)
    outf = mca.mca_out_ng(mca_obj=mf, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
    if rank == 0:
        res = {'kernel': kernel, 'capped': capped,
               'seeds_file': [mca.mca_inp_read(f)['Wld_jseed'] for f in sum(m.fnames_inp, [])],
               'seeds_fused': [mca.mca_inp_read(f)['Wld_jseed'] for f in sum(mf.fnames_inp, [])]}
        for v in ('rad', 'bt'):
            res['file_'+v] = out[v]['data']; res['fused_'+v] = outf[v]['data']
        solo = JobRunner(device=0); solo.rank, solo.world = 0, 1
        ir, ig = 1, 1
        r = run_job(m.fnames_inp[ir][ig], os.path.join(outdir, 'solo.bin'), int(m.photons[ir*m.Ng+ig]), 2, runner=solo)
        raw = mca.mca_out_raw(m.fnames_out[ir][ig])
        res['job_dist_rad'] = np.transpose(raw.data[0]['data'][:, :, :, 0], (2, 1, 0)); res['job_solo_rad'] = r['rad']
        np.savez(os.path.join(outdir, 'result.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
