"""-m gpu : the HIP path (through the C ABI) against the float64 oracle.

Bars:
  f64 entry points : 1e-9 * max(1,|ref|)   (same operation order as the oracle; only libm differs)
  f32 entry points : 1e-5 * max(1,|ref|)   (BASELINE.json north_star), arg-min / status exact
                     on every scenario that is not decided inside float32 noise.
Set-asides of the f32 comparisons (tools/f32_margin_probe.py measured them on 2048 scenarios / 65 536 rollouts:
the f32 entry agreed with the oracle on EVERY arg-min with no set-aside at all, and every rollout -- including those
with a stage argument within 1e-7 m of a curvature break-point -- stayed below 2.7e-6): a contender within F32_EPS = 1e-7
of a constraint threshold or of a break-point, or two best costs closer than F32_TIE = 1e-6.  The excluded share is
asserted (< 0.5 %) and printed.
"""
import os

import numpy as np
import pytest

import np_oracle as O
from igtmpc._lib import (DEV_ALL_ROWS, DEV_EXACT64, DEV_KEEP_QUEUES, DEV_NO_BOUND, DEV_NO_CAPTURE, DEV_NO_EARLY_EXIT, DEV_NO_FAR,
                         DEV_NO_PRUNE, DEV_NO_QUEUE_ORDER, DEV_NO_SEG_EMIT, DEV_NO_SLICES, DEV_NO_STEAL, DEV_NO_STEER_TABLE,
                         DEV_SEPARATE_QUEUES, DEV_STEER_SLICES, DEV_WAVES3, DEV_WHOLE_COLUMNS)
import parity_cases as PC
from helpers import F32_EPS, F32_TIE, REL_TOL, oracle_params, oracle_solve, rel_err, verdict_margins

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _batch(B, dtype, **kw):
    from igtmpc.scenarios import make_batch
    return make_batch(B, dtype=dtype, **kw)


def _args(b):
    return b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy']


def _cinf():
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes()


# ----------------------------------------------------------------------------- rollouts
def test_rollout_all_f64_matches_oracle(igt):
    b = _batch(96, np.float64)
    with igt.BatchSolver(dtype='f64') as s:
        P = oracle_params(s)
        s.set_cinf(*_cinf())
        got = s.rollout_all(*_args(b))
    ref = oracle_solve(b, P, cinf=_cinf())
    assert (ref['mask'] & 16).any(), 'sample never exercises the terminal set'
    assert rel_err(got['U'], ref['U']).max() == 0.0
    assert rel_err(got['X'], ref['X']).max() < 1e-9
    fin = np.isfinite(ref['J'])
    assert rel_err(got['cost'][fin], ref['J'][fin]).max() < 1e-9
    clear = np.abs(ref['g'] - P.feas_tol) > 1e-9
    assert ((got['viol'] == 0) == ref['feas'])[clear].all()
    assert (got['viol'][clear] == ref['mask'][clear]).all()


def test_rollout_all_f32_within_1e5(igt):
    b = _batch(96, np.float32)
    with igt.BatchSolver(dtype='f32') as s:
        P = oracle_params(s)
        s.set_cinf(*_cinf())
        got = s.rollout_all(*_args(b))
    ref = oracle_solve(b, P, cinf=_cinf())
    # controls are generated in double on the device and only rounded on store
    assert rel_err(got['U'], ref['U']).max() < 1e-7
    kp = b['kparams'].astype(np.float64)[:, None, :]
    x0 = O.apply_flags(b['x0'].astype(np.float64), b['flags'])[:, None, :]
    bp = O.breakpoint_distance(x0, ref['U'], kp, P)
    err = rel_err(got['X'], ref['X']).max(axis=(-1, -2))
    clear = bp > F32_EPS
    print(f'rollouts set aside (stage argument within {F32_EPS:g} m of a break-point): {(~clear).mean():.5f}')
    assert clear.mean() > 0.999, 'too many break-point-sensitive rollouts in the sample'
    assert err[clear].max() <= REL_TOL, f'max rel err {err[clear].max():.3e}'
    # a curvature switch decided inside float32 noise moves a trajectory by O(1e-3) at most
    assert err.max() < 5e-2
    cerr = rel_err(got['cost'], ref['J'])
    assert cerr[clear].max() <= REL_TOL
    thr = np.abs(ref['g'] - P.feas_tol) > 1e-6       # verdicts are formed in float from the double state
    assert ((got['viol'] == 0) == ref['feas'])[clear & thr].all()


# ----------------------------------------------------------------------------- solves
@pytest.mark.parametrize('dtype,tol,eps,eps_tie', [('f64', 1e-9, 1e-9, 1e-9), ('f32', REL_TOL, F32_EPS, F32_TIE)])
def test_solve_matches_oracle(igt, dtype, tol, eps, eps_tie):
    case = PC.solve_case(dtype)
    assert (tol, eps, eps_tie) == (case['tol'], case['eps'], case['tie'])
    with PC.open_solver(igt, case) as s:
        got = PC.device_solve(s, case)
    m = PC.check_case(case, got, PC.oracle_passes(case))
    assert 1.0 - m['compared'] / m['B'] < 0.005
    assert m['solved'] > 50, 'sample has too few solvable scenarios to mean anything'


@pytest.mark.parametrize('B,cand_mode,dtype', [(64, 'lattice', 'f32'), (64, 'ramp_hold', 'f32'), (2304, 'lattice', 'f32'),
                                               (64, 'lattice', 'f64'), (64, 'ramp_hold', 'f64'), (2304, 'lattice', 'f64'),
                                               (64, 'track', 'f32'), (2304, 'track', 'f32'), (9000, 'track', 'f32'), (2304, 'track', 'f64')])
def test_search_and_emit_agree_bitwise(igt, B, cand_mode, dtype):
    """emit re-rolls the winner with the arithmetic search used: the trajectory it stores must be exactly the
    rollout_all trajectory of that candidate.  f32: up to B = 2048 emit resumes four quarters of the horizon from the
    search pass's checkpoints (one lane each); above, it rolls the horizon in one piece: both must hold.  f64: search
    picks its sub-step variant by wave votes, emit uses the general one, rollout-all votes with other lane make-ups."""
    b = _batch(B, np.float32 if dtype == 'f32' else np.float64)
    with igt.BatchSolver(dtype=dtype, cand_mode=cand_mode) as s:
        s.set_cinf(*_cinf())
        sol = s.solve(*_args(b))
        n = min(B, 96)
        allc = s.rollout_all(*[a[:n] for a in _args(b)])
    assert (sol['argmin'][:n] >= 0).sum() > n // 2
    for i in range(n):
        c = sol['argmin'][i]
        if c >= 0:
            assert np.array_equal(sol['x'][i], allc['X'][i, c])
            assert np.array_equal(sol['u'][i], allc['U'][i, c])
            assert sol['cost'][i] == allc['cost'][i, c]
            assert allc['viol'][i, c] == 0


def test_f64_production_kernels_agree_with_oracle_order_kernels(igt, monkeypatch):
    """The float64 entry runs the factorised double arithmetic of igt_fast64.h on persistent waves; the kernels that
    follow the oracle operation for operation (ExactStepper<double>) stay in the library behind DEV_EXACT64.
    At BASELINE configs[1] size, where the numpy oracle is too slow to cover every scenario, the two must agree:
    same status everywhere, same arg-min except exact near-ties, trajectories and costs to 1e-11."""
    B = 4096
    b = _batch(B, np.float64)
    with igt.BatchSolver(dtype='f64') as s:
        s.set_cinf(*_cinf())
        fast = s.solve(*_args(b))
        allf = s.rollout_all(*[a[:64] for a in _args(b)])
    monkeypatch.setenv('IGT_DEV_FLAGS', str(DEV_EXACT64))
    with igt.BatchSolver(dtype='f64') as s:
        s.set_cinf(*_cinf())
        ref = s.solve(*_args(b))
        allr = s.rollout_all(*[a[:64] for a in _args(b)])
    assert np.array_equal(fast['status'], ref['status'])
    same = fast['argmin'] == ref['argmin']
    assert same.mean() > 0.999          # (and every difference is a tie of the two winners' costs to 1e-11: below)
    ok = same & (ref['status'] == 0)
    assert rel_err(fast['x'][ok], ref['x'][ok]).max() < 1e-11
    assert rel_err(fast['cost'][ok], ref['cost'][ok]).max() < 1e-11
    assert np.array_equal(fast['u'][ok], ref['u'][ok])
    # a different winner is only acceptable as a near-tie of the cost
    diff = ~same
    assert rel_err(fast['cost'][diff], ref['cost'][diff]).max(initial=0.0) < 1e-11
    # every candidate of 64 scenarios (infeasible ones included)
    assert rel_err(allf['X'], allr['X']).max() < 1e-11
    assert np.array_equal(allf['U'], allr['U'])
    fin = np.isfinite(allr['cost'])
    assert rel_err(allf['cost'][fin], allr['cost'][fin]).max() < 1e-11
    # a verdict bit may differ between the two arithmetics only where that verdict's worst margin sits on its threshold
    # (within 1e-9 of feas_tol, by the oracle's numbers for the same candidates)
    with igt.BatchSolver(dtype='f64') as s:
        P = oracle_params(s)
    A, bb = _cinf()
    Uo = allr['U'].astype(np.float64)
    X = O.rollout_frenet(O.apply_flags(b['x0'][:64], b['flags'][:64])[:, None, :], Uo, b['kparams'][:64, None, :], P)
    gm = verdict_margins(X, Uo, b['obs_xy'][:64, None], A, bb, P)
    diff_bits = allf['viol'] ^ allr['viol']
    for bit in (0, 1, 3, 4, 5):
        d = (diff_bits >> bit) & 1 == 1
        assert (np.abs(gm[..., bit][d] - P.feas_tol) < 1e-9).all(), (bit, int(d.sum()))
    assert (diff_bits & ~np.uint32(0b111011) == 0).all()
    assert (allf['viol'] == allr['viol']).mean() > 0.9995


# ----------------------------------------------------------------------------- golden vectors
def test_golden_frenet_rollouts_table_mode(igt, golden_dir):
    """Reference-generated rollouts (tests/golden/frenet_rk4_golden.npz) through the table
    candidate path: scenario i with table row i is the golden pair."""
    g = np.load(f'{golden_dir}/frenet_rk4_golden.npz')
    for dtype, npdt, tol in (('f64', np.float64, 1e-9), ('f32', np.float32, REL_TOL)):
        worst = 0.0
        with igt.BatchSolver(dtype=dtype, C=64, n_obs=0, cand_mode='table') as s:
            P = oracle_params(s)
            for lo in range(0, 1024, 64):
                sl = slice(lo, lo + 64)
                U = g['U'][sl]
                s.set_candidate_table(U)
                x0 = g['x0'][sl].astype(npdt)
                kp = g['kp'][sl].astype(npdt)
                out = s.rollout_all(x0, np.zeros((64, 2), npdt), kp, np.zeros(64, np.uint32),
                                    np.zeros((64, 0, 2, 21), npdt))
                got = out['X'][np.arange(64), np.arange(64)]
                if dtype == 'f64':
                    ref = g['X'][sl]
                    bp = np.full(64, np.inf)
                else:   # same (rounded) inputs through the oracle; golden pins the oracle itself
                    ref = O.rollout_frenet(x0.astype(np.float64), U, kp.astype(np.float64), P)
                    bp = O.breakpoint_distance(x0.astype(np.float64), U, kp.astype(np.float64), P)
                e = rel_err(got, ref).max(axis=(-1, -2))
                worst = max(worst, e[bp > F32_EPS].max())
        assert worst <= tol, f'{dtype}: {worst:.3e}'


def test_survey_known_answer(igt):
    """SURVEY.md section 4 KAT (reference model, recorded during the survey)."""
    k = np.arange(20)
    U = np.zeros((64, 2, 20))
    U[0] = np.stack([0.5 * np.cos(0.3 * k), 0.1 * np.sin(0.2 * k)])
    x0 = np.array([[18, 2.8, 18, 0.05, -0.02, 3, 0.0]])
    kp = np.array([[19.3, 19.3 + 8.6 * np.pi / 2, 1 / 8.6]])
    want20 = np.array([24.04054200868725, 3.1707601439799964, 23.768492505124048, -0.9596488518839958,
                       -0.47896770505284986, 2.9547762875359105, 0.06025930720195858])
    with igt.BatchSolver(dtype='f64', C=64, n_obs=0, cand_mode='table') as s:
        s.set_candidate_table(U)
        out = s.rollout_all(x0, np.zeros((1, 2)), kp, np.zeros(1, np.uint32), np.zeros((1, 0, 2, 21)))
    assert rel_err(out['X'][0, 0, :, 20], want20).max() < 1e-12


def test_golden_cartesian_euler(igt, golden_dir):
    g = np.load(f'{golden_dir}/cartesian_euler_golden.npz')
    with igt.BatchSolver(dtype='f64') as s:
        z = s.cartesian_euler(g['z'], g['u'][:, :, None])
    assert rel_err(z[:, :, 1], g['z_next']).max() < 1e-12
    with igt.BatchSolver(dtype='f32') as s:
        z = s.cartesian_euler(g['z'].astype(np.float32), g['u'][:, :, None].astype(np.float32))
    assert rel_err(z[:, :, 1], g['z_next']).max() < REL_TOL


# ----------------------------------------------------------------------------- edge cases
def test_empty_and_ragged_batches(igt):
    with igt.BatchSolver(dtype='f32') as s:
        e = _batch(8, np.float32)
        out = s.solve(*[a[:0] for a in _args(e)])
        assert out['x'].shape == (0, 7, 21)
        full = s.solve(*_args(e))
        for B in (1, 3, 5, 7):       # not multiples of the 4 scenarios a workgroup holds
            part = s.solve(*[a[:B] for a in _args(e)])
            for k in ('x', 'u', 'cost', 'argmin', 'status'):
                assert np.array_equal(part[k], full[k][:B], equal_nan=True)


def test_all_infeasible_reports_status_1(igt):
    b = _batch(16, np.float32)
    b['x0'][:, 3] = 0.5      # |ey_0| > 0.2 -> every candidate violates mpc.py:296-299 at k = 0
    with igt.BatchSolver(dtype='f32') as s:
        out = s.solve(*_args(b))
    assert (out['status'] == 1).all() and (out['argmin'] == -1).all()
    assert np.isnan(out['x']).all() and np.isinf(out['cost']).all()


@pytest.mark.parametrize('N,n_rk4,C,n_obs', PC.SHAPES_F64)
def test_other_shapes_f64(igt, N, n_rk4, C, n_obs):
    """... up to what include/igtmpc.h advertises: IGT_MAX_N = 64 (with the slice's steering table in LDS, C = 256 / 1024, and
    without, C = 64) and IGT_MAX_OBS = 4 obstacles.  From N = 40 on at limits under which the lattice has feasible members
    (parity_cases.LONG_LIMITS: at the reference's, no candidate of 64 steps stays in the lane and nothing would be compared);
    N = 33 is solved at the reference's own."""
    case = PC.shape_case('f64', N, n_rk4, C, n_obs)
    with PC.open_solver(igt, case) as s:
        got = PC.device_solve(s, case)
    PC.check_case(case, got, PC.oracle_passes(case))


def test_bad_arguments_fail_loudly(igt):
    with pytest.raises(igt.IgtError):
        igt.BatchSolver(C=100)
    with pytest.raises(igt.IgtError):
        igt.BatchSolver(N=0)
    with pytest.raises(igt.IgtError):
        igt.BatchSolver(C=576)          # 24 x 24 lattice does not tile 64 lanes
    # the limits' ranges (include/igtmpc.h igt_params): each refusal names the range it checks
    for bad, msg in ((dict(jerk_limit=0.0), 'jerk_limit must be in (0, inf)'), (dict(jerk_limit=-0.5), 'jerk_limit must be in (0, inf)'),
                     (dict(steer_rate_limit=-0.1), 'steer_rate_limit must be in [0, inf)'),
                     (dict(df_max=np.pi / 2), 'df_max must be in [0, pi/2)'), (dict(df_max=2.0), 'df_max must be in [0, pi/2)'),
                     (dict(dt=np.inf), 'must be finite'), (dict(v_max=np.inf), 'must be finite'), (dict(a_min=-np.inf), 'must be finite'),
                     (dict(jerk_limit=np.inf), 'must be finite'), (dict(ey_lim=np.nan), 'must be finite'),
                     (dict(w_u=np.inf), 'must be finite')):
        with pytest.raises(igt.IgtError, match=msg.replace('(', r'\(').replace(')', r'\)').replace('[', r'\[')):
            igt.BatchSolver(**bad)
    for edge in (dict(steer_rate_limit=0.0), dict(df_max=1.5), dict(jerk_limit=1e-3)):
        igt.BatchSolver(**edge).close()
    with igt.BatchSolver(cand_mode='table') as s:
        b = _batch(4, np.float32)
        with pytest.raises(igt.IgtError):
            s.solve(*_args(b))          # table never set


# ----------------------------------------------------------------------------- big batches / the other search build
@pytest.mark.parametrize('dtype,value_net', [('f32', False), ('f32', True), ('f64', False)])
def test_big_batch_and_other_build_equal_small_pieces(igt, golden_dir, monkeypatch, dtype, value_net):
    """The same scenarios solved in one ragged big batch (queues in index order, no longest-first sort), in small pieces
    (sorted queues, other queue make-up), and by the 3-waves-per-SIMD build of the persistent search kernel
    (DEV_WAVES3; a spilling build kept for A/B runs) must come out bit for bit the same -- with the progress
    cost and with the value network on the compact list (MFMA kernel, atomicMin winner)."""
    B = 24576 + 5                                  # not a multiple of 8: the last block of 8 has holes
    b = _batch(B, np.float32 if dtype == 'f32' else np.float64)
    kw = {}
    extra = []
    if value_net:
        layers = _nets(golden_dir)[3]
        kw = dict(cost_mode='value_net')
        extra = [b['tv_sv'], b['enc']]
    with igt.BatchSolver(dtype=dtype, **kw) as s:
        s.set_cinf(*_cinf())
        if value_net:
            s.set_value_net(layers)
        big = s.solve(*_args(b), *extra)
        cuts = [0, 4096, 8192, 8192 + 1003, 12288, 20000, B]
        parts = [s.solve(*[np.ascontiguousarray(a[lo:hi]) for a in list(_args(b)) + extra]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    monkeypatch.setenv('IGT_DEV_FLAGS', str(DEV_WAVES3))
    with igt.BatchSolver(dtype=dtype, **kw) as s3:
        s3.set_cinf(*_cinf())
        if value_net:
            s3.set_value_net(layers)
        other = s3.solve(*_args(b), *extra)
    for k in ('x', 'u', 'argmin', 'status', 'cost'):
        assert np.array_equal(np.concatenate([q[k] for q in parts]), big[k], equal_nan=True), k
        assert np.array_equal(other[k], big[k], equal_nan=True), k
    assert (big['status'] == 0).mean() > 0.5


# ----------------------------------------------------------------------------- full-size properties
def test_full_size_properties(igt):
    """BASELINE config 2 size (B=4096, C=256, N=20): size-independent properties."""
    import torch
    B = 4096
    b = _batch(B, np.float32)
    with igt.BatchSolver(dtype='f32') as s:
        s.set_cinf(*_cinf())
        base = s.solve(*_args(b))
        # (1) batch-permutation invariance
        perm = np.random.default_rng(0).permutation(B)
        p = s.solve(*[np.ascontiguousarray(a[perm]) for a in _args(b)])
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            assert np.array_equal(p[k], base[k][perm], equal_nan=True)
        # (2) shard concatenation == unsharded (the multi-GPU partition, 8 logical shards)
        parts = [s.solve(*[np.ascontiguousarray(a[i * 512:(i + 1) * 512]) for a in _args(b)]) for i in range(8)]
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            assert np.array_equal(np.concatenate([q[k] for q in parts]), base[k], equal_nan=True)
        # (3) device-resident buffers (torch tensors, current stream) == host staging
        dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in _args(b)]
        d = s.solve(*dev)
        torch.cuda.synchronize()
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            assert np.array_equal(d[k].cpu().numpy(), base[k], equal_nan=True)
        # (4) the winner is feasible and optimal among ALL candidates per the device's own table
        allc = s.rollout_all(*[a[:256] for a in _args(b)], want_X=False, want_U=False)
        J = np.where(allc['viol'] == 0, allc['cost'], np.inf)
        arg = J.argmin(axis=1)
        okk = np.isfinite(J.min(axis=1))
        assert (base['argmin'][:256][okk] == arg[okk]).all()
        assert (base['status'][:256] == np.where(okk, 0, 1)).all()
        # (5) trajectory is a rollout of its own controls (oracle, float64) on a sample
        P = oracle_params(s)
    idx = np.nonzero(base['status'] == 0)[0][:128]
    x0 = O.apply_flags(b['x0'][idx].astype(np.float64), b['flags'][idx])
    X = O.rollout_frenet(x0, base['u'][idx].astype(np.float64), b['kparams'][idx].astype(np.float64), P)
    bp = O.breakpoint_distance(x0, base['u'][idx].astype(np.float64), b['kparams'][idx].astype(np.float64), P)
    e = rel_err(base['x'][idx], X).max(axis=(-1, -2))
    assert e[bp > F32_EPS].max() <= REL_TOL


# ----------------------------------------------------------------------------- value network (gt_mpc, config 5)
def _nets(golden_dir):
    v = np.load(f'{golden_dir}/value_net_golden.npz')
    out = {}
    for sc in (1, 3):
        layers, i = [], 0
        while f'sc{sc}_W{i}' in v:
            layers.append((v[f'sc{sc}_W{i}'], v[f'sc{sc}_b{i}']))
            i += 1
        out[sc] = layers
    return out


@pytest.mark.parametrize('sc,dtype,tol,eps', [(1, 'f64', 1e-9, 1e-9), (3, 'f64', 1e-9, 1e-9),
                                              (1, 'f32', REL_TOL, 2e-5), (3, 'f32', REL_TOL, 2e-5)])
def test_value_net_cost_matches_oracle(igt, sc, dtype, tol, eps):
    """gt_mpc cost (mpc.py:367-369) with the shipped checkpoints V_GT_sc1 (2 hidden layers) and V_GT_sc3 (3),
    a non-trivial whitening / de-normalisation (synthetic: the reference's statistics are not shipped)."""
    case = PC.value_net_case(sc, dtype)
    assert (tol, eps, eps) == (case['tol'], case['eps'], case['tie'])
    a, net = case['args'], case['net']
    with igt.BatchSolver(dtype=dtype, cost_mode='value_net') as s:
        assert PC.params_equal(oracle_params(s), case['P'])
        s.set_cinf(*case['cinf'])
        with pytest.raises(igt.IgtError):
            PC.device_solve(s, case)          # net not loaded yet
        s.set_value_net(**net)
        got = PC.device_solve(s, case)
        pos, _ = PC.solve_args(case, 32)
        allc = s.rollout_all(*pos, want_X=False, want_U=False)
    oracle = PC.oracle_passes(case)
    ref = oracle[0][0]
    fin = np.isfinite(ref['J'][:32])
    assert rel_err(allc['cost'][fin], ref['J'][:32][fin]).max() <= tol
    m = PC.check_case(case, got, oracle)
    assert m['solved'] > 20
    # the terminal value really matters: it changes the winner w.r.t. the progress cost on this sample
    f = lambda k: np.asarray(a[k], dtype=np.float64)
    prog = O.solve_batch(f('x0'), f('u_prev'), f('kparams'), a['flags'], f('obs'), *case['cinf'], case['P'])
    sol = ref['status'] == 0
    assert (prog['argmin'][sol] != ref['argmin'][sol]).any()


# ----------------------------------------------------------------------------- ramp-hold candidates + refinement
@pytest.mark.parametrize('dtype,tol,eps', [('f64', 1e-9, 1e-9), ('f32', REL_TOL, 2e-5)])
def test_ramp_hold_with_refinement_matches_oracle(igt, dtype, tol, eps):
    """IGT_CAND_RAMP_HOLD with 2 refinement passes: every pass re-centres on the previous winner, so a scenario
    counts only if NO pass decided it inside float noise."""
    case = PC.ramp_hold_refined_case(dtype)
    assert (tol, eps, eps) == (case['tol'], case['eps'], case['tie'])
    with PC.open_solver(igt, case, refine=0) as s0:
        first = PC.device_solve(s0, case)
        pos, _ = PC.solve_args(case, 24)
        all0 = s0.rollout_all(*pos, want_X=False)
    with PC.open_solver(igt, case) as s2:
        got = PC.device_solve(s2, case)
    oracle = PC.oracle_passes(case)
    passes = oracle[0]
    # pass 0 alone
    assert rel_err(all0['U'], passes[0]['U'][:24]).max() < 1e-7
    PC.check_case(case, first, oracle, first=True)
    # after two refinements: the refined grids are so fine that near-ties are the rule; where every pass was
    # clear-cut the winner must be identical, elsewhere (ties only) the COST must agree
    m = PC.check_case(case, got, oracle)
    assert m['compared'] > 20
    # refinement never makes the answer worse, and improves it somewhere
    ref = passes[-1]
    both = (passes[0]['status'] == 0) & (ref['status'] == 0)
    assert (ref['cost'][both] <= passes[0]['cost'][both] + 1e-12).all()
    assert (ref['cost'][both] < passes[0]['cost'][both] - 1e-6).any()


@pytest.mark.parametrize('N,n_rk4,C,n_obs', PC.SHAPES_F32)
def test_other_shapes_f32(igt, N, n_rk4, C, n_obs):
    """float path at other discretisations (n_rk4 <= 2 switches to the longer offset polynomials), odd chunk
    counts (C = 64) and many slices (C = 1024).  From N = 40 on at limits under which the lattice has feasible members
    (parity_cases.LONG_LIMITS); N = 33 is solved at the reference's own."""
    case = PC.shape_case('f32', N, n_rk4, C, n_obs)
    with PC.open_solver(igt, case) as s:
        got = PC.device_solve(s, case)
    PC.check_case(case, got, PC.oracle_passes(case))


def test_value_net_with_ramp_hold_refinement_f64(igt):
    """gt_mpc cost + ramp-hold candidates + one refinement pass (per-chunk partials feed the refinement)."""
    case = PC.value_net_ramp_hold_case()
    with PC.open_solver(igt, case) as s:
        got = PC.device_solve(s, case)
    m = PC.check_case(case, got, PC.oracle_passes(case))
    assert m['solved'] > 10


@pytest.mark.parametrize('dtype,cand', [('f64', 'lattice'), ('f64', 'track'), ('f32', 'lattice'), ('f32', 'track')])
def test_production_kernel_switches_change_nothing(igt, dtype, cand, monkeypatch):
    """The A/B switches of the production kernels (IGT_DEV_FLAGS; VERDICT r2: "untested surface") only change HOW the work
    is laid out -- candidate slices in index order (1), no early exit (2), no steering table (4), no longest-first queues
    (16), no stealing between the XCDs' queues (512), tracking units cut along the steering axis (262144), units made of all
    acceleration rows instead of the live ones (2097152), the queues sorted by a launch of their own that knows the live rows
    instead of by the first workgroups of the acceleration-rows kernel (33554432) -- never the
    answer: every one of them gives the default solve bit for bit, on a batch small enough to take the queue builder."""
    npdt = np.float64 if dtype == 'f64' else np.float32
    b = _batch(1536, npdt)
    outs = {}
    for flag in (0, DEV_NO_SLICES, DEV_NO_EARLY_EXIT, DEV_NO_STEER_TABLE, DEV_NO_QUEUE_ORDER, DEV_NO_STEAL, DEV_STEER_SLICES,
                 DEV_ALL_ROWS, DEV_NO_BOUND, DEV_NO_SEG_EMIT, DEV_SEPARATE_QUEUES,
                 DEV_NO_SLICES | DEV_NO_EARLY_EXIT | DEV_NO_STEER_TABLE | DEV_NO_QUEUE_ORDER | DEV_NO_STEAL,
                 DEV_NO_STEER_TABLE | DEV_ALL_ROWS):
        monkeypatch.setenv('IGT_DEV_FLAGS', str(flag))
        with igt.BatchSolver(dtype=dtype, cand_mode=cand) as s:
            s.set_cinf(*_cinf())
            outs[flag] = s.solve(*_args(b))
    monkeypatch.delenv('IGT_DEV_FLAGS')
    # igt_set_concurrency: the search kernels take one wave per SIMD when the caller overlaps solves -- same answers
    with igt.BatchSolver(dtype=dtype, cand_mode=cand) as s:
        s.set_cinf(*_cinf())
        s.set_concurrency(4)
        outs['concurrency 4'] = s.solve(*_args(b))
        for bad in (0, -3, 65):
            with pytest.raises(igt.IgtError):
                s.set_concurrency(bad)
    assert (outs[0]['status'] == 0).mean() > 0.5
    for flag, o in outs.items():
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            assert np.array_equal(o[k], outs[0][k], equal_nan=True), (flag, k)


@pytest.mark.parametrize('cand,N,C,B', [('lattice', 20, 256, 4096), ('ramp_hold', 20, 256, 4096), ('track', 20, 256, 4096),
                                        ('lattice', 20, 256, 8200), ('track', 40, 256, 1500), ('lattice', 40, 256, 1500),
                                        ('lattice', 20, 1024, 700), ('track', 12, 1024, 700), ('ramp_hold', 20, 64, 4500),
                                        ('lattice', 12, 4096, 200), ('track', 8, 4096, 120), ('track', 20, 256, 16500),
                                        ('track', 20, 64, 9000), ('lattice', 64, 256, 1100), ('lattice', 64, 64, 4200),
                                        ('ramp_hold', 64, 256, 1100), ('track', 64, 256, 1100)])
def test_units_of_live_acceleration_rows_change_nothing(igt, golden_dir, cand, N, C, B, monkeypatch):
    """The f64 search first rolls the G acceleration recurrences of every scenario (accel_rows_kernel) and builds its units from
    the rows that hold the speed box and the terminal set -- a failing row is infeasible in all of its columns, so it cannot
    win (igt_kernels_f64.hip "Acceleration rows that cannot win").  With DEV_ALL_ROWS every row is rolled as
    before: the solve must be the same bit for bit -- with and without the queue builder (B = 8200 has none), at both horizons,
    with 1, 4, 16 and 64 units per scenario, with warm starts and a refinement pass, and under the value-network cost.  (Batches of
    up to two rounds of units -- 1024 scenarios at 256 candidates -- keep the plain layout: every size here is above that.)
    The tracking family's default solve also prunes against the scenario's incumbent (igt_fast64.h BOUND: units of the highest
    acceleration rows first, a later unit's candidates are lost once a lower bound of their cost exceeds the best cost a finished
    unit has left): with all rows rolled there is no such pass, with DEV_NO_BOUND the bound alone is off -- the same
    bits, with the queue order table (B <= 6144) and with unit-rank-major item decoding (B = 8200, 16 500)."""
    b = _batch(B, np.float64, N=N)
    rng = np.random.default_rng(11)
    flags, u_prev, u_ws = b['flags'], b['u_prev'], None
    if cand != 'lattice':      # two thirds of the scenarios carry a warm start (its base sequence moves the rows' recurrences)
        prev = O.candidates_lattice(b['u_prev'], O.Params(N=N))[np.arange(B), (np.arange(B) * 37) % 256]
        u_ws = np.ascontiguousarray(O.shift_controls(prev))
        u_prev = np.ascontiguousarray(prev[:, :, 0])
        flags = flags | np.where(np.arange(B) % 3 != 0, 2, 0).astype(np.uint32)
    for cost_mode in ('progress', 'value_net'):
        if cost_mode == 'value_net' and (C != 256 or B > 4096):
            continue
        outs = []
        net = dict(layers=_nets(golden_dir)[1], Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)), mu_f=np.zeros(6), sigma_t=2.0, mu_t=0.3)
        # live rows, 64 per unit (tracking: + the incumbent bound); all rows; live rows in whole columns; (tracking:) no incumbent bound
        # ... ; the queue builder as a launch of its own (where the batch has one)
        for flag in (0, DEV_ALL_ROWS, DEV_WHOLE_COLUMNS) + ((DEV_NO_BOUND,) if cand == 'track' else ()) + ((DEV_SEPARATE_QUEUES,) if B <= 4500 else ()):
            monkeypatch.setenv('IGT_DEV_FLAGS', str(flag))
            with igt.BatchSolver(N=N, C=C, dtype='f64', cand_mode=cand, cost_mode=cost_mode,     # (tracking at N = 40: with a refinement
                                 refine_iters=1 if (cand == 'ramp_hold' or (cand == 'track' and N == 40)) else 0) as s:   # pass -- the incumbents restart)
                s.set_cinf(*_cinf())
                extra = ()
                if cost_mode == 'value_net':
                    s.set_value_net(**net)
                    extra = (b['tv_sv'], b['enc'])
                outs.append(s.solve(b['x0'], u_prev, b['kparams'], flags, b['obs_xy'], *extra, u_ws=u_ws))
        monkeypatch.delenv('IGT_DEV_FLAGS')
        assert (outs[0]['status'] == 0).mean() > (0.3 if N <= 40 else 0.0)      # (over 64 steps few lattice candidates stay in the lane)
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            for o in outs[1:]:
                assert np.array_equal(outs[0][k], o[k], equal_nan=True), (cost_mode, k)


@pytest.mark.parametrize('cand,N,n_rk4,C,B', [('lattice', 20, 4, 256, 4096), ('track', 20, 4, 256, 4096), ('ramp_hold', 20, 4, 256, 1500),
                                              ('table', 20, 4, 256, 700), ('track', 40, 4, 256, 900), ('lattice', 13, 3, 64, 2100),
                                              ('track', 9, 2, 1024, 300), ('ramp_hold', 64, 4, 256, 500), ('lattice', 8, 4, 256, 8200)])
def test_emit_in_pieces_is_the_emit_in_one_piece(igt, cand, N, n_rk4, C, B, monkeypatch):
    """Batches that do not keep trajectories emit the winner in four pieces of the horizon, each resumed from a checkpoint the
    search pass left (igt_fast64.h SEGMODE; emit_seg_f64_kernel), the Cartesian rows rolled on their own from the controls, the
    outputs written as contiguous lines.  With DEV_NO_SEG_EMIT emit_f64_kernel rolls the winner in one piece as before:
    the same x, u, cost, arg-min, status bit for bit -- every family, horizons that are and are not multiples of four, both
    sub-step builds, the coarse discretisation's long polynomials, warm starts and a refinement pass, 1 to 16 units per
    scenario; and the winner's trajectory is rollout-all's for the same candidate, bit for bit."""
    rng = np.random.default_rng(3)
    b = _batch(B, np.float64, N=N)
    table = None
    if cand == 'table':
        a, d = np.meshgrid(np.linspace(-0.25, 0.25, 16), np.linspace(-0.04, 0.04, 16), indexing='ij')
        table = np.ascontiguousarray(np.stack([a.ravel(), d.ravel()], axis=1)[:, :, None] * np.ones(N) + 1e-3 * rng.normal(size=(256, 2, N)))
    flags, u_prev, u_ws = b['flags'], b['u_prev'], None
    if cand in ('ramp_hold', 'track'):
        prev = O.candidates_lattice(b['u_prev'], O.Params(N=N))[np.arange(B), (np.arange(B) * 37) % 256]
        u_ws = np.ascontiguousarray(O.shift_controls(prev))
        u_prev = np.ascontiguousarray(prev[:, :, 0])
        flags = flags | np.where(np.arange(B) % 3 != 0, 2, 0).astype(np.uint32)
    outs, alls = [], None
    for flag in (0, DEV_NO_SEG_EMIT):
        monkeypatch.setenv('IGT_DEV_FLAGS', str(flag))
        with igt.BatchSolver(N=N, n_rk4=n_rk4, C=C, dtype='f64', cand_mode=cand, refine_iters=1 if cand == 'ramp_hold' else 0) as s:
            s.set_cinf(*_cinf())
            if table is not None:
                s.set_candidate_table(table)
            outs.append(s.solve(b['x0'], u_prev, b['kparams'], flags, b['obs_xy'], u_ws=u_ws))
            if flag == 0 and cand != 'ramp_hold':      # (a refinement pass re-centres the candidates: rollout-all rolls the first pass)
                alls = s.rollout_all(b['x0'][:48], u_prev[:48], b['kparams'][:48], flags[:48], b['obs_xy'][:48], u_ws=None if u_ws is None else u_ws[:48])
    monkeypatch.delenv('IGT_DEV_FLAGS')
    assert (outs[0]['status'] == 0).any() and (outs[0]['status'] == 1).any()
    for k in ('x', 'u', 'cost', 'argmin', 'status'):
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
    if alls is not None:
        for i in range(48):
            cw = outs[0]['argmin'][i]
            if cw >= 0:
                assert np.array_equal(outs[0]['x'][i], alls['X'][i, cw]) and np.array_equal(outs[0]['u'][i], alls['U'][i, cw]), i


@pytest.mark.parametrize('cand,N', [('lattice', 20), ('track', 20), ('ramp_hold', 20), ('track', 40), ('table', 20)])
def test_kept_trajectories_are_the_rerolled_ones(igt, cand, N, monkeypatch):
    """Double batches with no more 64-candidate units than the chip has SIMDs (256 scenarios at 256 candidates): the search
    pass keeps every candidate's trajectory and emit copies the winner's (igt_kernels_common.h CaptureSink,
    emit_gather_f64_kernel) instead of rolling it again.  With the capture switched off (DEV_NO_CAPTURE:
    emit_f64_kernel re-rolls) the solve is the same bit for bit -- at B = 1, 33 (ragged last block of 8) and 256, for every
    candidate family, at both horizons.  Every unit of such a batch gets a wave of its own instead of a place in the XCDs'
    queues (search_is_static; DEV_KEEP_QUEUES keeps the queues): same bits again."""
    rng = np.random.default_rng(5)
    table = None
    if cand == 'table':
        a, d = np.meshgrid(np.linspace(-0.25, 0.25, 16), np.linspace(-0.04, 0.04, 16), indexing='ij')     # held controls
        table = np.ascontiguousarray(np.stack([a.ravel(), d.ravel()], axis=1)[:, :, None] * np.ones(N) +
                                     1e-3 * rng.normal(size=(256, 2, N)))
    full = _batch(256, np.float64, N=N)
    for B in (1, 33, 256):
        b = {k: np.ascontiguousarray(v[:B]) for k, v in full.items()}
        outs = []
        for flag in (0, DEV_NO_CAPTURE, DEV_KEEP_QUEUES):      # default; re-rolled by emit; kept, but with the unit queues
            monkeypatch.setenv('IGT_DEV_FLAGS', str(flag))
            with igt.BatchSolver(N=N, dtype='f64', cand_mode=cand) as s:
                s.set_cinf(*_cinf())
                if table is not None:
                    s.set_candidate_table(table)
                outs.append(s.solve(*_args(b)))
        monkeypatch.delenv('IGT_DEV_FLAGS')
        if B == 256:
            assert (outs[0]['status'] == 0).mean() > 0.1
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), (B, k)
            assert np.array_equal(outs[0][k], outs[2][k], equal_nan=True), (B, k)


@pytest.mark.parametrize('cost_mode,refine', [('value_net', 0), ('progress', 2)])
def test_kept_trajectories_with_value_net_and_refinement(igt, golden_dir, cost_mode, refine, monkeypatch):
    """Same as above where the winner is not the search pass's own: chosen by the terminal value network after the pass
    (gt_mpc), or by the last of three ramp-hold passes (each pass overwrites the kept trajectories)."""
    b = _batch(200, np.float64)
    cand = 'track' if cost_mode == 'value_net' else 'ramp_hold'
    outs = []
    for flag in (0, DEV_NO_CAPTURE):
        monkeypatch.setenv('IGT_DEV_FLAGS', str(flag))
        with igt.BatchSolver(dtype='f64', cost_mode=cost_mode, cand_mode=cand, refine_iters=refine) as s:
            s.set_cinf(*_cinf())
            if cost_mode == 'value_net':
                s.set_value_net(layers=_nets(golden_dir)[3], Wn=np.eye(6), mu_f=np.zeros(6), sigma_t=1.0, mu_t=0.0)
                outs.append(s.solve(*_args(b), b['tv_sv'], b['enc']))
            else:
                outs.append(s.solve(*_args(b)))
    monkeypatch.delenv('IGT_DEV_FLAGS')
    assert (outs[0]['status'] == 0).mean() > 0.5
    for k in ('x', 'u', 'cost', 'argmin', 'status'):
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k


@pytest.mark.parametrize('dtype,cand', [('f64', 'lattice'), ('f64', 'track'), ('f32', 'lattice'), ('f32', 'ramp_hold')])
def test_cartesian_row_skip_changes_nothing(igt, dtype, cand, monkeypatch):
    """Search units whose obstacles are out of every speed-feasible candidate's reach roll without x, y (igt_device.h
    obstacles_out_of_reach; 70 % of the benchmark batch).  The switched-off build path (DEV_NO_FAR) must give the
    same solve bit for bit -- on the benchmark batch, on a batch whose obstacle sits just inside / just outside the reach
    bound, with two obstacles of which one is near, and with three and four (IGT_MAX_OBS)."""
    npdt = np.float64 if dtype == 'f64' else np.float32
    b = _batch(1024, npdt)
    far = (np.hypot(b['obs_xy'][:, 0, 0, 1:] - b['x0'][:, None, 0], b['obs_xy'][:, 0, 1, 1:] - b['x0'][:, None, 1]).min(axis=1) > 17.5)
    assert 0.5 < far.mean() < 0.9                                  # both kinds of unit are exercised
    # obstacles parked at the reach bound 5.6 + 20 * 0.1 * (5 + 4 * 0.1) + 1 = 17.4 m from the start, +- a little
    edge = {k: v.copy() for k, v in b.items()}
    ang = np.linspace(0, 2 * np.pi, 1024, endpoint=False)
    r = 17.4 + np.tile(np.array([-0.5, -1e-6, 1e-6, 0.5]), 256)
    edge['obs_xy'][:, 0, 0, :] = (b['x0'][:, 0] + r * np.cos(ang))[:, None]
    edge['obs_xy'][:, 0, 1, :] = (b['x0'][:, 1] + r * np.sin(ang))[:, None]
    two = {k: v[:256].copy() for k, v in b.items()}
    two['obs_xy'] = np.concatenate([b['obs_xy'][:256], np.full_like(b['obs_xy'][:256], -20.0)], axis=1)
    # three and four obstacles (IGT_MAX_OBS): far ones around a near or a far first one, the last one parked at the reach bound
    many = {}
    for n in (3, 4):
        many[n] = {k: v[:256].copy() for k, v in b.items()}
        extra = [np.full_like(b['obs_xy'][:256], 40.0 + 5.0 * m) for m in range(n - 2)] + [edge['obs_xy'][:256]]
        many[n]['obs_xy'] = np.ascontiguousarray(np.concatenate([b['obs_xy'][:256]] + extra, axis=1))
    for batch, n_obs in ((b, 1), (edge, 1), (two, 2), (many[3], 3), (many[4], 4)):
        outs = []
        for flag in (0, DEV_NO_FAR):
            monkeypatch.setenv('IGT_DEV_FLAGS', str(flag))
            with igt.BatchSolver(dtype=dtype, cand_mode=cand, n_obs=n_obs) as s:
                s.set_cinf(*_cinf())
                outs.append(s.solve(*_args(batch)))
        monkeypatch.delenv('IGT_DEV_FLAGS')
        assert (outs[0]['status'] == 0).any()
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k


@pytest.mark.parametrize('sc', [1, 3])
def test_value_bound_pruning_changes_nothing(igt, golden_dir, sc, monkeypatch):
    """gt_mpc cost, tracking candidates (long lists of feasible candidates): the list is pruned with an interval bound on
    the value network before the matrix-core kernel runs (value_bound_kernel / value_prune_kernel).  Entries that are dropped
    cannot win, so the solve with pruning == the solve without (DEV_NO_PRUNE), bit for bit -- with a non-trivial
    whitening and a NEGATIVE sigma_t as well (the bound takes the upper end whatever the sign)."""
    nets = PC.value_bound_nets(sc)
    b = _batch(768, np.float64)
    for net in nets:
        outs = []
        for flag in (0, DEV_NO_PRUNE):
            monkeypatch.setenv('IGT_DEV_FLAGS', str(flag))
            with igt.BatchSolver(dtype='f64', cost_mode='value_net', cand_mode='track') as s:
                s.set_cinf(*_cinf())
                s.set_value_net(**net)
                outs.append(s.solve(*_args(b), b['tv_sv'], b['enc']))
        monkeypatch.delenv('IGT_DEV_FLAGS')
        assert (outs[0]['status'] == 0).mean() > 0.5
        for k in ('x', 'u', 'cost', 'argmin', 'status'):
            assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
    # ... and the pruned solve is the oracle's answer (one scenario subset, sigma_t = 1)
    case = PC.value_bound_case(sc)
    with PC.open_solver(igt, case) as s:
        got = PC.device_solve(s, case)
    PC.check_case(case, got, PC.oracle_passes(case))


# ----------------------------------------------------------------------------- warm start (augment_prev_sol)
@pytest.mark.parametrize('dtype,tol,eps', [('f64', 1e-9, 1e-9), ('f32', REL_TOL, 2e-5)])
def test_warm_started_ramp_hold_matches_oracle(igt, dtype, tol, eps):
    """igt_solve_batch_ws_* / igt_rollout_batch_ws_*: ramp-hold targets centred on a warm start (the previous solution
    shifted by one step, utils.py:354-363) where flags carry IGT_FLAG_WARM, on u_prev held elsewhere; one refinement
    pass on top.  Every candidate's controls and trajectory, then the solve."""
    case = PC.warm_case(dtype, 'ramp_hold')
    assert (tol, eps, eps) == (case['tol'], case['eps'], case['tie'])
    a, P = case['args'], case['P']
    u_ws, flags = a['u_ws'], a['flags']
    with PC.open_solver(igt, case, refine=0) as s0:
        pos, kw = PC.solve_args(case, 48)
        all0 = s0.rollout_all(*pos, **kw)
        first = PC.device_solve(s0, case)
    with PC.open_solver(igt, case) as s1:
        got = PC.device_solve(s1, case)
    oracle = PC.oracle_passes(case)
    passes, x0, kp = oracle
    r0 = passes[0]
    # the warm start itself is candidate (G/2, G/2) wherever the scenario carries one
    w = (flags & 2) != 0
    assert rel_err(r0['U'][w, 8 * 16 + 8], u_ws[w]).max() < 1e-7
    assert not np.allclose(r0['U'][~w, 8 * 16 + 8], u_ws[~w])
    assert rel_err(all0['U'], r0['U'][:48]).max() <= (1e-14 if dtype == 'f64' else 1e-7)
    bp = O.breakpoint_distance(x0[:48], r0['U'][:48], kp[:48], P)
    clear = bp > eps
    err = rel_err(all0['X'], r0['X'][:48]).max(axis=(-1, -2))
    assert err[clear].max() <= tol
    m0 = PC.check_case(case, first, oracle, first=True)
    assert m0['solved'] > 30
    # refined pass: costs agree wherever no threshold / break-point decided a pass inside float noise
    PC.check_case(case, got, oracle)
    # a warm start needs the ramp-hold family
    with igt.BatchSolver(dtype=dtype) as s2:
        with pytest.raises(igt.IgtError):
            pos, kw = PC.solve_args(case)
            s2.solve(*pos, **kw)


# ----------------------------------------------------------------------------- tracking candidates (state-feedback steering)
@pytest.mark.parametrize('dtype,tol,eps', [('f64', 1e-9, 1e-9), ('f32', REL_TOL, 2e-5)])
def test_tracking_candidates_match_oracle(igt, dtype, tol, eps):
    """IGT_CAND_TRACK: ramp-hold accelerations, steering as a state feedback evaluated inside the roll-out
    (beta_cmd = -epsi - k_e ey + offset_j, rate-limited).  The controls come out of the roll-out, so every candidate's
    controls AND trajectory are compared with the oracle's interleaved generation; then the solve, with a warm start on
    two thirds of the scenarios and one refinement pass; and the family must beat ramp-hold on its own cost."""
    case = PC.warm_case(dtype, 'track')
    assert (tol, eps, eps) == (case['tol'], case['eps'], case['tie'])
    P = case['P']
    with PC.open_solver(igt, case, refine=0) as s0:
        assert (s0.params.track_ke, s0.params.track_span, s0.params.track_beta_lim, s0.params.track_env) == (0.3, 0.1, 0.7, 1.0)
        pos, kw = PC.solve_args(case, 48)
        all0 = s0.rollout_all(*pos, **kw)
        first = PC.device_solve(s0, case)
    with PC.open_solver(igt, case) as s1:
        got = PC.device_solve(s1, case)
    with PC.open_solver(igt, dict(case, cand='ramp_hold'), refine=0) as s2:
        rh = PC.device_solve(s2, case)
    oracle = PC.oracle_passes(case)
    passes, x0, kp = oracle
    r0 = passes[0]
    bp = O.breakpoint_distance(x0[:48], r0['U'][:48], kp[:48], P)
    clear = bp > eps
    # the steering depends on the rolled state: f64 agrees to rounding, f32 to the trajectory tolerance
    assert rel_err(all0['U'][clear], r0['U'][:48][clear]).max() <= (1e-12 if dtype == 'f64' else REL_TOL)
    assert rel_err(all0['X'], r0['X'][:48]).max(axis=(-1, -2))[clear].max() <= tol
    # steering differs between the accelerations of one offset column (it is placed, not timed)
    assert np.abs(r0['U'][:, 0 * 16 + 8, 1] - r0['U'][:, 15 * 16 + 8, 1]).max() > 1e-3
    m0 = PC.check_case(case, first, oracle, first=True)
    assert m0['solved'] > 60
    PC.check_case(case, got, oracle)
    # quality: solves more scenarios than ramp-hold and costs less where both solve
    assert (first['status'] == 0).sum() >= (rh['status'] == 0).sum()
    both = (first['status'] == 0) & (rh['status'] == 0)
    assert first['cost'][both].mean() < rh['cost'][both].mean() - 0.05


def test_tracking_steering_feedback_over_its_whole_range(igt):
    """The steering command atan(tan(beta)/r) is evaluated on the device as atan2(sin beta, r cos beta) with an interval
    reduction of its own (igt_math64.h): with |beta| allowed up to 1.4 rad, offsets of +-1.2 rad and a lateral gain of 2
    every interval of the reduction (|t| up to 11.6) and the range-reduced sincos are exercised; every candidate's
    controls must still be the numpy oracle's np.arctan(np.tan(beta)/r) chain to 1e-12."""
    B = 64
    b = _batch(B, np.float64)
    f = lambda k: np.asarray(b[k], dtype=np.float64)
    args = (b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'])
    tk = dict(ke=2.0, span=1.2, blim=1.4)
    with igt.BatchSolver(dtype='f64', cand_mode='track', track_ke=tk['ke'], track_span=tk['span'], track_beta_lim=tk['blim']) as s:
        P = oracle_params(s)
        s.set_cinf(*_cinf())
        all_ = s.rollout_all(*args)
    ref = O.solve_batch_refined(f('x0'), f('u_prev'), f('kparams'), b['flags'], f('obs_xy'), *_cinf(), P, cand='track', track=tk)[0]
    x0 = O.apply_flags(f('x0'), b['flags'])[:, None, :]
    clear = O.breakpoint_distance(x0, ref['U'], f('kparams')[:, None, :], P) > 1e-9
    d = ref['U'][:, :, 1, :]
    assert np.abs(d).max() > 0.99 and (np.abs(np.diff(d, axis=-1)).max() > 0.069)      # box and rate limits are reached
    assert rel_err(all_['U'][clear], ref['U'][clear]).max() <= 1e-12
    fin = clear & np.isfinite(ref['X']).all(axis=(-1, -2))
    assert rel_err(all_['X'][fin], ref['X'][fin]).max() <= 1e-9


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_tracking_speed_cap_matches_oracle(igt, dtype):
    """igt_params.track_vcap (default on): the acceleration targets stay under the largest a_k from which a jerk-limited ramp
    still keeps v <= v_max (igt_device.h track_speed_cap; oracle np_oracle.track_speed_cap).  Scenarios that start near the
    speed limit (v0 = 3.6 .. 4.9 m/s) so that the top rows meet the cap: every candidate's controls and the solve agree with the
    oracle with the cap on and off, capped candidates stay inside the speed box, and the cap never makes an answer worse."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    res = {}
    for vcap in (1.0, 0.0):
        case = PC.speed_cap_case(dtype, vcap)
        x0, u_prev, P, eps = case['args']['x0'], case['args']['u_prev'], case['P'], case['eps']
        with PC.open_solver(igt, case) as s:
            assert s.params.track_vcap == vcap
            pos, _ = PC.solve_args(case, 32)
            all_ = s.rollout_all(*pos)
            got = PC.device_solve(s, case)
        oracle = PC.oracle_passes(case)
        ref = oracle[0][0]
        clear = O.breakpoint_distance(oracle[1][:32], ref['U'][:32], oracle[2][:32], P) > eps
        assert rel_err(all_['U'][clear], ref['U'][:32][clear]).max() <= (1e-12 if dtype == 'f64' else 2e-5)
        m = PC.check_case(case, got, oracle)
        assert m['solved'] > 30
        res[vcap] = (got, ref)
    got1, ref1 = res[1.0]
    got0, ref0 = res[0.0]
    # the highest acceleration row under the cap: inside the speed box over the whole horizon, at v_max - margin at the end
    a_top1, a_top0 = ref1['U'][:, 15 * 16 + 8, 0, :], ref0['U'][:, 15 * 16 + 8, 0, :]
    v1 = f(x0)[:, 5:6] + np.cumsum(P.dt * a_top1, axis=1)
    v0 = f(x0)[:, 5:6] + np.cumsum(P.dt * a_top0, axis=1)
    # (where the initial (v, a) still allows it: from v0 = 4.9 with a = 1.2 no jerk-limited ramp stays under the limit)
    ctrl = O.track_speed_cap(f(x0)[:, 5], P) >= f(u_prev)[:, 0] - P.dt * P.jerk
    assert ctrl.mean() > 0.5 and v1[ctrl].max() <= P.v_max - O.TRACK_VCAP_MARGIN + 1e-9
    assert (v0.max(axis=1) > P.v_max + 0.05).mean() > 0.8
    both = (ref1['status'] == 0) & (ref0['status'] == 0)
    assert both.sum() > 40 and (ref1['cost'][both] <= ref0['cost'][both] + 1e-12).all()
    assert (ref1['cost'][both] < ref0['cost'][both] - 1e-3).mean() > 0.3          # ... and often better
    gb = (got1['status'] == 0) & (got0['status'] == 0)
    assert (got1['cost'][gb] < got0['cost'][gb] - 1e-3).mean() > 0.3


@pytest.mark.parametrize('env', [0.0, 0.5])
def test_tracking_envelope_scale_matches_oracle(igt, env):
    """igt_params.track_env: 0 switches the acceleration envelope off (constant targets), any other scale moves the
    line E_k = env dt^2 (N - k - 1/2) / (2 w_u); every candidate's controls and the solve agree with the oracle run at
    the same scale, and the scale changes the answer.  A negative scale is refused."""
    case = PC.envelope_case(env)
    P = case['P']
    f = lambda k: np.asarray(case['args'][k], dtype=np.float64)
    with PC.open_solver(igt, case) as s:
        pos, _ = PC.solve_args(case, 32)
        all_ = s.rollout_all(*pos)
        got = PC.device_solve(s, case)
    with PC.open_solver(igt, dict(case, limits={}, P=PC.host_params(), tk=PC.host_track())) as s1:
        dflt = PC.device_solve(s1, case)
    oracle = PC.oracle_passes(case)
    ref = oracle[0][0]
    clear = O.breakpoint_distance(oracle[1][:32], ref['U'][:32], oracle[2][:32], P) > 1e-9
    assert rel_err(all_['U'][clear], ref['U'][:32][clear]).max() <= 1e-12
    slope = O.track_env_slope(P, env)
    E = slope * (P.N - np.arange(P.N) - 0.5)
    a = ref['U'][:, :, 0, :]
    a_before = np.concatenate([np.broadcast_to(f('u_prev')[:, None, 0, None], a.shape[:2] + (1,)), a[..., :-1]], axis=-1)
    # above the line a candidate can only be on its way down at the jerk limit
    assert (a <= np.maximum(E, a_before - P.dt * P.jerk) + 1e-12).all()
    m = PC.check_case(case, got, oracle)
    assert m['solved'] > 30
    both = (got['status'] == 0) & (dflt['status'] == 0)
    assert np.abs(got['cost'][both] - dflt['cost'][both]).max() > 1e-3
    with pytest.raises(Exception):
        igt.BatchSolver(dtype='f64', cand_mode='track', track_env=-1.0)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_exact_ties_across_slices_resolve_to_the_lowest_index(igt, dtype):
    """Steering-ordered slices hold their columns from the centre outwards, so of EXACTLY tied candidates the lowest
    index can sit in the LAST slice.  Construction: a vehicle at rest with v_max = 0 and no control-effort
    weight -- only the 16 candidates that keep a = 0 are feasible, steering changes nothing, all 16 tie exactly; the
    winner must be candidate (i = 8, j = 0) = 128, which the steering order puts into the last slice (a reduction that
    trusted the slice order would return (8, 8) = 136)."""
    npdt = np.float64 if dtype == 'f64' else np.float32
    B = 96
    b = _batch(B, npdt)
    b['x0'][:, 5] = 0.0
    b['u_prev'][:, 0] = 0.0
    f = lambda k: np.asarray(b[k], dtype=np.float64)
    none = np.zeros((B, 0, 2, 21), npdt)
    with igt.BatchSolver(dtype=dtype, cand_mode='ramp_hold', n_obs=0, v_max=0.0, w_u=0.0) as s:
        P = oracle_params(s)
        got = s.solve(b['x0'], b['u_prev'], b['kparams'], b['flags'], none)
        allc = s.rollout_all(b['x0'][:8], b['u_prev'][:8], b['kparams'][:8], b['flags'][:8], none[:8], want_X=False, want_U=False)
    ref = O.solve_batch_refined(f('x0'), f('u_prev'), f('kparams'), b['flags'], none.astype(np.float64), None, None, P)[0]
    assert (ref['feas'].sum(axis=1) == 16).all() and (ref['argmin'] == 128).all()
    assert all(len(np.unique(ref['J'][i, ref['feas'][i]])) == 1 for i in range(B)), 'the 16 feasible candidates must tie exactly'
    assert ((allc['viol'] == 0).sum(axis=1) == 16).all()
    assert all(len(np.unique(allc['cost'][i, allc['viol'][i] == 0])) == 1 for i in range(8))
    assert (got['status'] == 0).all() and (got['argmin'] == 128).all()
