"""-m gpu : the HIP path at BASELINE.json's FULL configuration sizes, through the C ABI.

  configs[2]  batch = 65 536 scenarios (all 8 sc variants tiled), horizon 20, Frenet model
  configs[3]  262 144 scenarios sharded 8 ways  -> the shard one GPU solves: 32 768 (rank 3's block here)
  configs[4]  gt_mpc: batch = 65 536 with the terminal value network in the cost

The oracle's full [B, C, 7, N+1] tensor would be ~20 GB at these sizes, so each test
  (1) compares a FIXED 512-scenario subsample taken from inside the big batch's result with the float64
      oracle run on exactly those scenarios (f64: 1e-9, f32: 1e-5, arg-min / status exact where the decision
      is not inside float noise), and
  (2) checks over the WHOLE batch the size-independent property the domain offers: scenarios are independent,
      so the big batch must equal the same scenarios solved in pieces, bit for bit.
"""
import numpy as np
import pytest

import parity_cases as PC
from helpers import F32_EPS, REL_TOL

pytestmark = pytest.mark.gpu

ARGS = ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy')


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _check_pieces(solver, b, big, cuts, extra=()):
    """big batch == the same scenarios solved in pieces (different queue make-up, other search build), bitwise."""
    keys = list(ARGS) + list(extra)
    parts = [solver.solve(*[np.ascontiguousarray(b[k][lo:hi]) for k in keys]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for k in ('x', 'u', 'cost', 'argmin', 'status'):
        assert np.array_equal(np.concatenate([q[k] for q in parts]), big[k], equal_nan=True), k


def _run(igt, name, B, offset, dtype, tol, eps, gt_sc=0, cand='lattice'):
    """The subsample, its set-aside widths and its recorded floors are parity_cases.fullsize_case's."""
    case, idx, b = PC.fullsize_case(name, B, offset, dtype, gt_sc, cand)
    assert (tol, eps) == (case['tol'], case['eps'])
    assert set(np.unique(b['sc'])) == set(range(1, 9)), 'all 8 scenario variants must be tiled into the batch'
    extra = ('tv_sv', 'enc') if gt_sc else ()
    with PC.open_solver(igt, case) as s:
        big = s.solve(*[b[k] for k in list(ARGS) + list(extra)])
        assert 0.5 < (big['status'] == 0).mean() < 1.0
        q = B // 4
        _check_pieces(s, b, big, [0, 4096, 4096 + 1003, q + 17, 2 * q, 3 * q + 5, B], extra)
    got = {k: big[k][idx] for k in ('x', 'u', 'cost', 'argmin', 'status')}
    m = PC.check_case(case, got, PC.oracle_passes(case))
    # the bounds this file has always asserted, next to the recorded ones
    assert m['compared'] / m['B'] > (0.99 if cand == 'lattice' else 0.85), 'too little of the subsample is decided outside float noise'
    assert m['solved'] > 100, 'subsample has too few solvable scenarios to mean anything'


@pytest.mark.parametrize('dtype,tol,eps', [('f64', 1e-9, 1e-9), ('f32', REL_TOL, F32_EPS)])
def test_config2_batch_65536(igt, dtype, tol, eps):
    """BASELINE configs[2]: batch = 65 536, all 8 sc variants tiled, horizon 20, Frenet-frame model."""
    _run(igt, 'config2', 65536, 0, dtype, tol, eps)


@pytest.mark.parametrize('dtype,tol,eps', [('f64', 1e-9, 1e-9), ('f32', REL_TOL, F32_EPS)])
def test_config3_shard_32768(igt, dtype, tol, eps):
    """BASELINE configs[3]: 262 144 scenarios sharded 8 ways = 32 768 per GPU; rank 3's shard (offset 3 x 32 768,
    the generator's per-rank offset path).  The all-gather across ranks is covered by tests/test_sharding_gloo.py."""
    _run(igt, 'config3', 32768, 3 * 32768, dtype, tol, eps)


@pytest.mark.parametrize('dtype,tol,eps,sc', [('f64', 1e-9, 1e-9, 1), ('f64', 1e-9, 1e-9, 3), ('f32', REL_TOL, F32_EPS, 1),
                                              ('f32', REL_TOL, F32_EPS, 3)])
def test_config4_gt_mpc_65536(igt, golden_dir, dtype, tol, eps, sc):
    """BASELINE configs[4]: gt_mpc, terminal value network (shipped V_GT_sc1: 2 hidden layers, V_GT_sc3: 3) evaluated
    on the GPU inside the cost, batch = 65 536 (per GPU; the 8-GPU run itself is the driver's)."""
    _run(igt, 'config4', 65536, 0, dtype, tol, eps, sc)


@pytest.mark.parametrize('dtype,tol,eps', [('f64', 1e-9, 1e-9), ('f32', REL_TOL, 2e-5)])
def test_config2_batch_65536_tracking_family(igt, dtype, tol, eps):
    """The same full-size batch through the family the planner and the closed-loop driver use by default
    (IGT_CAND_TRACK: steering feedback inside the roll-out, acceleration envelope): oracle on the 512-scenario subsample
    + the big batch equals the same scenarios solved in pieces, bitwise."""
    _run(igt, 'config2_track', 65536, 0, dtype, tol, eps, cand='track')
