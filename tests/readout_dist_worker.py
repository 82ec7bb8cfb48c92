"""
Worker of tests/test_gpu_readout.py::test_two_ranks_batched_thermal_files_match_one_rank: one process per rank under
torch.distributed.run, backend 'gloo', both ranks on the ONE GPU of a test box.  Thermal flux and thermal satellite radiance over a
synthetic cloud field, two g x two runs, files kept and no abs_obj: mca_run hands such jobs to JobRunner.run_batched (one all-reduce per
batch, rank 0 normalises the rows in torch).  Rank 0 then runs every input file again alone, and all ranks run the fused route over the
same job files.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P tests/readout_dist_worker.py <outdir>
"""
import contextlib
import copy
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
    from er3t_amd.rtm.mca.mca_exe import JobRunner, run_job
    from tests.golden import inputs as gin

    batched = [0]
    run_batched = JobRunner.run_batched

    def counting(self, *a, **k):
        batched[0] += 1
        return run_batched(self, *a, **k)
    JobRunner.run_batched = counting

    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(11000.0, atm, Ng=2)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(outdir, 'atm3d.bin'), quiet=True)
    res = {}
    solo = None
    for target in ('flux', 'radiance'):
        kw = dict(sensor_zenith_angle=[0.0, 26.1], sensor_azimuth_angle=[0.0, 0.0]) if target == 'radiance' else {}
        batched[0] = 0
        m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target=target, source='thermal', surface_albedo=0.02, Nrun=2, photons=4e5,
                           weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True,
                           fdir=os.path.join(outdir, target), **kw)
        res[target+'_batched'] = batched[0]
        # the fused route over the SAME job files (their seeds): run statistics on the device, one all-reduce per run
        mf = copy.copy(m)
        mf.abs_obj, mf.keep_files, mf.fused = ab, False, None
        mf.run_fused()
        if rank == 0:
            res[target+'_njob'] = m.Nrun*m.Ng
            files = mca.mca_out_ng(mca_obj=m, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
            fused = mca.mca_out_ng(mca_obj=mf, abs_obj=ab, mode='mean', squeeze=True, quiet=True).data
            for k in ('f_up', 'f_down') if target == 'flux' else ('rad',):
                res['%s_files_%s' % (target, k)] = files[k]['data']; res['%s_fused_%s' % (target, k)] = fused[k]['data']
            if solo is None:
                solo = JobRunner(device=0); solo.rank, solo.world = 0, 1
            for ir in range(m.Nrun):
                for ig in range(m.Ng):
                    j = ir*m.Ng+ig
                    r = run_job(m.fnames_inp[ir][ig], os.path.join(outdir, 'solo_%s%d.bin' % (target, j)), int(m.photons[j]), 0, runner=solo)
                    raw = mca.mca_out_raw(m.fnames_out[ir][ig])
                    sc = solo.scene
                    res['%s_factor_%d' % (target, j)] = solo.sol.source_power()[0]/((sc.dx*sc.nx)*(sc.dy*sc.ny)*sc.mu0)
                    if target == 'flux':
                        for v in range(3):
                            res['flux_dist_%d_%d' % (j, v)] = raw.data[v]['data'][..., 0]
                            res['flux_solo_%d_%d' % (j, v)] = np.transpose(r['flux'][v], (2, 1, 0))
                    else:
                        res['radiance_dist_%d_0' % j] = raw.data[0]['data'][..., 0]
                        res['radiance_solo_%d_0' % j] = np.transpose(r['rad'], (2, 1, 0))
    if rank == 0:
        np.savez(os.path.join(outdir, 'result.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
