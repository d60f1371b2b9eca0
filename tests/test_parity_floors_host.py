"""No GPU: the floors the GPU parity tests assert, held to their inputs by the oracle alone.

Every comparison that goes through helpers.compare_solve (test_gpu_parity.py, test_gpu_fullsize.py, every seed of
test_gpu_fuzz.py, the draws of test_gpu_limits.py, the lanes' subsamples of test_gpu_overlap.py) builds its inputs without a solver (parity_cases.all_cases).  Here the numpy
oracle runs on the same inputs and its compared share, its share outside thresholds and break-points and its count of solved
and compared scenarios must be at least what tests/golden/parity_floors.json records (tools/parity_floors.py --write) -- so a
recorded figure cannot drift from the inputs, and a reviewer can check every floor on a machine without a GPU.

The numpy oracle takes ten seconds and more on the larger batches.  Of the cases in parity_cases.HOST_SUBSAMPLED the first 130
scenarios are measured, here and by the tool: fuzz seeds 19, 21, 36, 38, 110, 203, 204 and 206, solve, ramp_hold_refined[f64],
config2, config3, config4 (all of them) and config2_track[f64].  Each of these is compared whole (share 1.0), so the share of a
part is the batch's and the solved count of a part is a lower bound; cases with set-asides are measured in full."""
import json
import os

import pytest

import parity_cases as PC
import test_gpu_limits as L
from helpers import floors

KEYS = [k for k, _ in PC.all_cases()]
with open(os.path.join(PC.GOLDEN, 'parity_floors.json')) as _fh:
    RECORDED = json.load(_fh)['cases']


@pytest.mark.parametrize('key', KEYS)
def test_recorded_floors_hold_on_the_inputs(key):
    for k, m in PC.measure_key(key).items():
        rec = RECORDED[k]
        print(f'{k}: measured {m}, recorded {rec}')
        assert m['B'] == rec['B']
        assert m['compared'] >= rec['compared'] and m['tie_compared'] >= rec['tie_compared'], (k, m, rec)
        assert m['solved'] >= rec['min_solved'], (k, m, rec)
        if not k.endswith('/first'):
            # what the issue of the floors asks of the inputs themselves: enough solved scenarios to compare (12 for a shape, 8
            # for a fuzz draw or half of a batch under 16), a winner across a curvature break-point at the long horizons
            assert rec['min_solved'] >= m['need'], (k, rec, m['need'])
            assert m['crossing'] >= m['crossing_needed'], (k, m)
        if m['f64'] and rec['compared'] < rec['B']:
            # ... and the reason names the rule that the measurement says set the scenarios aside
            why = rec.get('why', '')
            assert why, f'{k}: a float64 share below 1 needs its reason recorded'
            edges, ties = m['tie_compared'] < m['B'], m['compared'] < m['tie_compared']
            assert why.startswith('near-ties alone') == (ties and not edges), (k, why, m)
            assert why.startswith(('threshold set-asides alone', 'break-point set-asides alone')) == (edges and not ties), (k, why, m)
        else:
            assert 'why' not in rec, f'{k}: a reason is recorded for a share that needs none'
        assert floors(k)['min_solved'] == rec['min_solved']


def test_every_recorded_case_is_a_case():
    names = set(KEYS) | {k + '/first' for k in KEYS}
    assert set(RECORDED) <= names, set(RECORDED) - names
    assert set(KEYS) <= set(RECORDED)


@pytest.mark.parametrize('dtype,seeds', [('f64', range(L.N_SEEDS)), ('f32', L.F32_SEEDS)])
def test_limits_share_table_is_the_recorded_one(dtype, seeds):
    """test_gpu_limits.py keeps its shares (and the reason for each) in its own table: they must not exceed what is measured."""
    for seed in seeds:
        rec = RECORDED[f'limits[{seed}-{dtype}]']
        assert rec['compared'] / rec['B'] >= L.SHARE.get((dtype, seed), 1.0) - 5e-4, (dtype, seed, rec)
