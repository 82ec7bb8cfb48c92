"""
bench.py without and with --full: a plain run prints the headline line alone (the steps, their rate and the configuration);
--full adds what is measured or checked beyond it (here the roofline object, the CPU leg switched off and its keys null).
"""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEYOND_THE_HEADLINE = ('roofline', 'cpu_baseline', 'parity', 'secondary', 'published_case', 'strong')


def _line(extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--photons', '2e6',
                        '--workload', 'les128'] + extra, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_adds_the_rest():
    plain = _line([])
    assert plain['full'] is False and not any(k in plain for k in BEYOND_THE_HEADLINE)
    assert (plain['metric'], plain['unit'], plain['dtype'], plain['higher_is_better']) == ('photons/sec', 'photons/s', 'f32', True)
    assert plain['steps'] == 2 and plain['warmup'] == 1 and plain['value'] > 0.0
    assert abs(plain['value']*plain['ms_per_step']*1.0e-3 - 2.0e6) < 1.0                 # one step = --photons histories
    assert plain['config']['photons_per_step'] == 2000000 and plain['config']['mean_radiance'] > 0.0

    full = _line(['--full', '--no-cpu-baseline', '--no-pmc'])
    assert full['full'] is True and full['cpu_baseline'] is None and full['parity'] is None
    assert full['roofline']['bytes_per_photon'] > 0.0 and full['roofline']['launches'] > 0
    assert full['roofline']['per_photon']['scatter'] > 0.0
    assert set(plain) == set(full) - set(BEYOND_THE_HEADLINE)
