"""No GPU: what the oracle alone says about the per-scenario candidate cases (tests/candidate_cases.py) that
tests/test_gpu_candidates.py compares the device against.  helpers.measure with eps = tie = 1e-9: every scenario of every case is
compared -- none is set aside --, the solved count and the winners that cross a curvature break-point are the figures the GPU
test asks for, and the OR of the verdict bits over a case shows every verdict raised somewhere."""
import numpy as np
import pytest

import candidate_cases as CC
import np_oracle as O
from helpers import measure


@pytest.mark.parametrize('key', list(CC.CASES), ids=CC.case_id)
def test_oracle_figures(key):
    case, want = CC.build(key), CC.CASES[key]
    passes, x0, kp = CC.oracle(case)
    m, amb, edge = measure(passes, case['P'], x0, kp, CC.BAR, CC.BAR)
    print(CC.case_id(key), m)
    assert m['compared'] == m['tie_compared'] == m['B'] == case['B'], m      # no scenario may be set aside
    assert m['solved'] == want['solved'], m
    assert m['crossing'] == want['crossing'], m
    bits = int(np.bitwise_or.reduce(passes[0]['mask'].ravel()))
    assert bits == want['bits'], bits


def test_generator_breaks_rate_and_box_in_every_scenario():
    case = CC.build(next(iter(CC.CASES)))
    U, P, C, N = case['U'], case['P'], case['C'], case['N']
    assert U.shape == (case['B'], C, 2, N)
    ra = P.dt * P.jerk
    prev = np.concatenate([np.broadcast_to(case['u_prev'][:, None, 0, None], U.shape[:2] + (1,)), U[:, :, 0, :-1]], axis=-1)
    rate = (np.abs(U[:, :, 0] - prev) - ra).max(axis=-1) > P.feas_tol
    box = (U[:, :, 0].max(axis=-1) - P.a_max) > P.feas_tol
    assert rate[:, C - C // 8:].all() and box[:, C - C // 16:].all()
    assert not rate[:, :C - C // 8].any() and not box[:, :C - C // 8].any()
    # scenarios differ: no two of them share a candidate set
    assert len({U[b].tobytes() for b in range(case['B'])}) == case['B']


def test_oracle_takes_a_table_per_scenario():
    """solve_batch(U=[B,C,2,N]) answers scenario b as it does alone with the shared table U[b]."""
    case = CC.build((24, 13, 128, 0, 4, False, None))
    ref = CC.oracle(case)[0][0]
    A, b = case['cinf']
    for i in (0, 7, 23):
        sl = slice(i, i + 1)
        one = O.solve_batch(case['x0'][sl], case['u_prev'][sl], case['kparams'][sl], case['flags'][sl], None, A, b, case['P'],
                            C=case['C'], U=case['U'][i], return_all=True)
        assert one['argmin'][0] == ref['argmin'][i] and one['status'][0] == ref['status'][i]
        assert one['cost'].tobytes() == ref['cost'][sl].tobytes() and one['J'].tobytes() == ref['J'][sl].tobytes()
