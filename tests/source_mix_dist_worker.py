"""
Worker of tests/test_gpu_source_mix.py::test_two_ranks_match_one: one process per rank under torch.distributed.run, backend 'gloo', both
ranks on the ONE GPU of a test box.  A radiance and a heating-rate simulation with the solar+thermal source (Src_mtype = 2) over a
synthetic cloud field through the file route -- job by job: run, all-reduce of the raw tallies, the mi3d_get_* read-outs with the mixed
job's own amplitude --; rank 0 then runs every job file again alone.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P tests/source_mix_dist_worker.py <outdir>
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
    from er3t_amd.rtm.mca.mca_exe import JobRunner, run_job
    from tests.golden import inputs as gin

    atm = atm_synth(np.concatenate([np.arange(0, 11)*0.2, np.arange(3, 21)*1.0]))
    ab = abs_synth(3750.0, atm, Ng=2)
    ab.coef['solar']['data'] = np.array([9.0, 11.0])*1.0e-3          # W m-2 nm-1: sunlight and emission of the same size at 3.75 um
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(outdir, 'atm3d.bin'), quiet=True)
    res = {}
    solo = None
    for target in ('radiance', 'heating rate'):
        key = target.split()[0]
        m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target=target, source='solar+thermal', surface_albedo=0.2,
                           solar_zenith_angle=40.0, solar_azimuth_angle=30.0, Nrun=2, photons=2e5, weights=ab.coef['weight']['data'],
                           solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True, fdir=os.path.join(outdir, key))
        if rank == 0:
            if solo is None:
                solo = JobRunner(device=0); solo.rank, solo.world = 0, 1
            res['njob_'+key] = m.Nrun*m.Ng
            for ir in range(m.Nrun):
                for ig in range(m.Ng):
                    j = ir*m.Ng+ig
                    r = run_job(m.fnames_inp[ir][ig], os.path.join(outdir, 'solo_%s%d.bin' % (key, j)), int(m.photons[j]), 0, runner=solo)
                    raw = mca.mca_out_raw(m.fnames_out[ir][ig])
                    if key == 'radiance':
                        res['dist_rad_%d' % j] = raw.data[0]['data'][..., 0]; res['solo_rad_%d' % j] = np.transpose(r['rad'], (2, 1, 0))
                    else:
                        res['dist_hrt_%d' % j] = raw.data[3]['data'][..., 0]; res['solo_hrt_%d' % j] = np.transpose(r['heat'], (2, 1, 0))
                        for iv, name in enumerate(('fdnd', 'fdn', 'fup')):
                            res['dist_%s_%d' % (name, j)] = raw.data[iv]['data'][..., 0]
                            res['solo_%s_%d' % (name, j)] = np.transpose(r['flux'][iv], (2, 1, 0))
                        res['emission_max'] = max(res.get('emission_max', 0.0), float(solo.sol.emission().max()))
                    res['kernel_'+key] = solo.sol.kernel_name()
    if rank == 0:
        np.savez(os.path.join(outdir, 'result.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
