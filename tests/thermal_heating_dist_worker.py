"""
Worker of tests/test_gpu_thermal_heating.py::test_two_ranks_match_one: one process per rank under torch.distributed.run, backend
'gloo', both ranks on the ONE GPU of a test box.  Net heating rates of a thermal job (Flx_mhrt = 2) over a synthetic cloud field through
the file route -- job by job: run, all-reduce of the raw tallies, mi3d_get_heating --; rank 0 then runs every job file again alone.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P tests/thermal_heating_dist_worker.py <outdir>
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
    ab = abs_synth(11000.0, atm, Ng=2)
    cld = cld_synth(atm, nx=12, ny=10, nz=10, z_base=0.4, z_top=1.6, cot_mean=8.0, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        a1 = mca.mca_atm_1d(atm_obj=atm, abs_obj=ab)
        a3 = mca.mca_atm_3d(atm_obj=atm, cld_obj=cld, fname=os.path.join(outdir, 'atm3d.bin'), quiet=True)
    m = mca.mcarats_ng(atm_1ds=[a1], atm_3ds=[a3], Ng=2, target='heating rate', source='thermal', surface_albedo=0.02, Nrun=2, photons=4e5,
                       weights=ab.coef['weight']['data'], solver='3D', mp_mode='py', overwrite=True, date=gin.DATE, quiet=True,
                       fdir=os.path.join(outdir, 'file'))
    if rank == 0:
        res = {'njob': m.Nrun*m.Ng}
        solo = JobRunner(device=0); solo.rank, solo.world = 0, 1
        emax = 0.0
        for ir in range(m.Nrun):
            for ig in range(m.Ng):
                j = ir*m.Ng+ig
                r = run_job(m.fnames_inp[ir][ig], os.path.join(outdir, 'solo%d.bin' % j), int(m.photons[j]), 0, runner=solo)
                raw = mca.mca_out_raw(m.fnames_out[ir][ig])
                res['dist_hrt_%d' % j] = raw.data[3]['data'][..., 0]; res['solo_hrt_%d' % j] = np.transpose(r['heat'], (2, 1, 0))
                res['dist_fup_%d' % j] = raw.data[2]['data'][..., 0]; res['solo_fup_%d' % j] = np.transpose(r['flux'][2], (2, 1, 0))
                emax = max(emax, float(solo.sol.emission().max()))
        res['emission_max'] = emax
        np.savez(os.path.join(outdir, 'result.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
