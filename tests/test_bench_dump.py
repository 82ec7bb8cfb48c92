"""
bench.py --dump-outputs: what the timed path computed in its last step, as .npy files that two builds can be compared on.
CPU: the writer (dtypes, the 64 MB bound, the seeded sample) and the argument checks.  GPU: the files hold the LAST timed step --
its photon ids are fixed by --warmup + --steps alone, so two runs that end on the same step write the same outputs and a run that
ends one step earlier does not.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    return {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}


def test_dump_writes_small_outputs_whole(tmp_path):
    import bench
    f = np.random.default_rng(1).random((2, 5, 7)).astype(np.float32)
    t = f.astype(np.float64)*3.0
    written = bench.dump_outputs(str(tmp_path), {'radiance': f, 'tally': t})
    assert written == {'radiance.npy': [2, 5, 7], 'tally.npy': [2, 5, 7]}
    g, u = np.load(str(tmp_path/'radiance.npy')), np.load(str(tmp_path/'tally.npy'))
    assert g.dtype == np.float32 and u.dtype == np.float64
    assert np.array_equal(g, f) and np.array_equal(u, t)
    assert not (tmp_path/'sample_index.npy').exists()


def test_dump_samples_large_outputs_within_the_bound_and_the_same_in_every_run(tmp_path):
    import bench
    n = 3*117*200*200
    f = np.arange(n, dtype=np.float32)
    t = np.arange(n, dtype=np.float64)
    limit = 4*10**6                                  # (the bound scaled down: same code path as 64 MB against a 480 x 480 flux job)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path/d), {'flux': f, 'tally': t}, limit=limit)
        assert sum(os.path.getsize(str(tmp_path/d/x)) for x in os.listdir(str(tmp_path/d))) <= limit
    idx = np.load(str(tmp_path/'a'/'sample_index.npy'))
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(str(tmp_path/'b'/'sample_index.npy')))
    assert idx.size > 0.9*limit/(8 + 4 + 8) and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(np.load(str(tmp_path/'a'/'flux.npy')), f[idx.astype(np.int64)])
    assert np.array_equal(np.load(str(tmp_path/'a'/'tally.npy')), t[idx.astype(np.int64)])


def test_dump_refuses_other_dtypes(tmp_path):
    import bench
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path), {'counts': np.arange(4)})


@pytest.mark.parametrize('argv', [['--steps', '0'], ['--warmup', '-1']])
def test_bench_refuses_no_timed_steps(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--dry-run'] + argv, capture_output=True, text=True, timeout=300,
                       env=_env())
    assert r.returncode != 0 and '--steps must be at least 1' in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """(steps 3, warmup 1) and (steps 1, warmup 3) end on the same photon ids and must write the same images up to the order of the
    float additions; (steps 2, warmup 1) ends one step earlier, on other photons.  The normalised field is the tally of ONE step
    of --photons histories times Src_flx mu0 nxr nyr / photons."""
    import bench

    def run(steps, warmup):
        d = tmp_path/('s%d_w%d' % (steps, warmup))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                            '--photons', '2e6', '--workload', 'les128', '--no-cpu-baseline', '--no-secondary', '--no-pmc',
                            '--dump-outputs', str(d)], capture_output=True, text=True, timeout=600, env=_env())
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
        assert line['steps'] == steps and line['warmup'] == warmup
        rad, tally = np.load(str(d/'radiance.npy')), np.load(str(d/'tally.npy'))
        assert rad.dtype == np.float32 and tally.dtype == np.float64 and rad.shape == tally.shape
        return rad, tally

    scene = bench.make_scene('les128')
    a, ta = run(3, 1)
    b, tb = run(1, 3)
    c, _ = run(2, 1)
    assert a.shape == (scene.nview, scene.nyr, scene.nxr) and np.all(np.isfinite(a)) and a.max() > 0.0
    fac = scene.src_flx*scene.mu0*scene.nxr*scene.nyr/2.0e6
    assert np.allclose(a, ta*fac, rtol=1e-6, atol=1e-7*a.max())
    assert np.allclose(a, b, rtol=1e-4, atol=1e-6*a.max()) and np.allclose(ta, tb, rtol=1e-4, atol=1e-6*ta.max())
    assert np.abs(a-c).max() > 1e-2*a.max()
