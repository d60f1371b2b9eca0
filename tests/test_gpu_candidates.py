"""Per-scenario candidate sets on the device: BatchSolver.solve_candidates / rollout_candidates on U[B,C,2,N]
(include/igtmpc.h igt_solve_candidates_f64 / igt_rollout_candidates_f64).

  1. the same bits as the shared table: row b is what a table handle whose table is U[b] answers for scenario b, byte for byte
     -- solve and roll-out, progress cost, its polish and the value-network cost, the staged kernel (N = 20) and the direct one
     (N = 40);
  2. parity with the oracle on the seven cases of tests/candidate_cases.py (tests/test_candidate_cases_host.py holds their
     figures to the inputs): no scenario set aside, tol = eps = tie = 1e-9;
  3. isolation: a scenario whose U is all NaN answers status 1, every other row is byte-equal to the clean solve;
  4. device tensors: captured in a stream graph, a replay reads what U holds then;
  5. what is refused, and that an empty batch and a handle without a shared table work."""
import contextlib
import ctypes

import numpy as np
import pytest

import candidate_cases as CC
from helpers import compare_solve, rel_err, verdict_margins
from parity_cases import LONG_LIMITS, cinf_default, value_net_case

pytestmark = pytest.mark.gpu

SOLVE_KEYS = ('x', 'u', 'cost', 'argmin', 'status')
ROLL_KEYS = ('X', 'U', 'cost', 'viol')


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ----------------------------------------------------------------------------- 1. the same bits as the shared table
def _six_scenarios(N, limits):
    """Six scenarios of make_batch -- turning and straight routes, one with the other vehicle in reach --, C = 128 candidates
    each: scenario 1's first unit is made infeasible (its winner sits in the second unit), scenario 4 entirely."""
    from igtmpc.scenarios import make_batch
    from helpers import host_params
    b = make_batch(64, dtype=np.float64, N=N)
    P = host_params(N=N, **limits)
    d = np.sqrt(((b['obs_xy'][:, 0, :, :] - b['x0'][:, :2, None]) ** 2).sum(axis=1)).min(axis=-1)
    turning, near = b['kparams'][:, 2] != 0, d < 8.0
    pick = list(np.flatnonzero(turning)[:2]) + list(np.flatnonzero(~turning)[:2])
    pick += [i for i in np.flatnonzero(near) if i not in pick][:1]
    pick += [i for i in range(64) if i not in pick][:6 - len(pick)]
    pick = np.asarray(pick)
    assert len(pick) == 6 and turning[pick].any() and (~turning[pick]).any() and near[pick].any()
    a = {k: np.ascontiguousarray(b[k][pick]) for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc')}
    U = CC.per_scenario_candidates(a['u_prev'], P, 128, N)
    U[1, :64, 0, 3] = P.a_max + 0.5
    U[4, :, 0, 3] = P.a_max + 0.5
    return a, U


@pytest.mark.parametrize('N', [20, 40])
@pytest.mark.parametrize('mode', ['progress', 'polish', 'value'])
def test_same_bits_as_the_shared_table(igt, mode, N):
    limits = dict(LONG_LIMITS) if N == 40 else {}
    a, U = _six_scenarios(N, limits)
    net = value_net_case(1, 'f64')['net'] if mode == 'value' else None
    kw = dict(limits, polish_iters=1) if mode == 'polish' else limits
    pos = [a['x0'], a['u_prev'], a['kparams'], a['flags']]
    opt = dict(obs_xy=a['obs_xy'])
    if net:
        opt.update(tv_sv=a['tv_sv'], enc=a['enc'])
    with igt.BatchSolver(N=N, C=128, dtype='f64', cand_mode='table', cost_mode='value_net' if net else 'progress', **kw) as s:
        s.set_cinf(*cinf_default())
        if net:
            s.set_value_net(**net)
        got = s.solve_candidates(*pos, U, **opt)
        roll = s.rollout_candidates(*pos, U, **opt)
        for b in range(6):
            s.set_candidate_table(U[b])
            one = s.solve(*pos, **opt)
            for k in SOLVE_KEYS:
                assert _same_bytes(one[k][b], got[k][b]), (mode, N, b, k)
            all_ = s.rollout_all(*pos, **opt)
            for k in ROLL_KEYS:
                assert _same_bytes(all_[k][b], roll[k][b]), (mode, N, b, k)
    print(mode, N, 'status', got['status'], 'argmin', got['argmin'])
    assert got['status'][4] == 1 and got['argmin'][4] == -1 and np.isposinf(got['cost'][4]) and np.isnan(got['x'][4]).all()
    assert got['status'][1] == 0 and got['argmin'][1] >= 64, 'scenario 1 must be won in the second unit'
    assert (got['status'] == 0).sum() >= 2      # (the oracle solves three of the six at N = 20, two at N = 40)
    assert (roll['viol'][4] & 2).all() and (roll['viol'][:, 112:] & 4).all()      # input box; rate limit (the last eighth)


# ----------------------------------------------------------------------------- 2. oracle parity
@pytest.mark.parametrize('key', list(CC.CASES), ids=CC.case_id)
def test_matches_the_oracle(igt, key):
    case, want = CC.build(key), CC.CASES[key]
    passes, x0, kp = CC.oracle(case)
    ref, P = passes[0], case['P']
    pos, opt = CC.solve_args(case)
    with CC.open_solver(igt, case) as s:
        got = s.solve_candidates(*pos, case['U'], **opt)
        roll = s.rollout_candidates(*pos, case['U'], **opt)
    compare_solve(got, passes, P, x0, kp, eps=CC.BAR, tie=CC.BAR, tol=CC.BAR, share=1.0, tie_share=1.0,
                  min_solved=want['solved'], crossing=want['crossing'], label='candidates[' + CC.case_id(key) + ']')
    # every candidate of every scenario (as test_rollout_all_f64_matches_oracle)
    assert rel_err(roll['U'], ref['U']).max() == 0.0
    assert rel_err(roll['X'], ref['X']).max() < 1e-9
    fin = np.isfinite(ref['J'])
    worst = rel_err(roll['cost'][fin], ref['J'][fin]).max()
    print('rollout_candidates: worst cost error', worst)
    assert worst <= 1e-9
    A, b = case['cinf']
    g = verdict_margins(ref['X'], ref['U'], case['obs'][:, None] if case['n_obs'] else None, A, b, P)
    clear = (np.abs(g - P.feas_tol) > CC.BAR).all(axis=-1)
    assert clear.mean() > 0.99
    assert (roll['viol'][clear] == ref['mask'][clear]).all()
    assert ((roll['viol'] == 0) == ref['feas'])[clear].all()


# ----------------------------------------------------------------------------- 3. isolation
@pytest.mark.parametrize('key', [(24, 20, 256, 1, 4, False, None), (24, 40, 64, 2, 4, True, None), (24, 20, 128, 1, 4, False, 1)],
                         ids=CC.case_id)
def test_a_poisoned_candidate_set_stays_in_its_scenario(igt, key):
    case = CC.build(key)
    pos, opt = CC.solve_args(case)
    clean_ref = CC.oracle(case)[0][0]
    b0 = int(np.flatnonzero(clean_ref['status'] == 0)[1])      # a scenario that is solved on clean candidates
    bad = case['U'].copy()
    bad[b0] = np.nan
    with CC.open_solver(igt, case) as s:
        clean = s.solve_candidates(*pos, case['U'], **opt)
        got = s.solve_candidates(*pos, bad, **opt)
        roll = s.rollout_candidates(*pos, bad, want_X=False, want_U=False, **opt)
    assert clean['status'][b0] == 0
    assert got['status'][b0] == 1 and got['argmin'][b0] == -1 and np.isposinf(got['cost'][b0])
    assert np.isnan(got['x'][b0]).all() and np.isnan(got['u'][b0]).all()
    assert (roll['viol'][b0] != 0).all()
    others = np.arange(case['B']) != b0
    for k in SOLVE_KEYS:
        assert _same_bytes(got[k][others], clean[k][others]), k


# ----------------------------------------------------------------------------- 4. device tensors and capture
@contextlib.contextmanager
def _side_stream(torch):
    """A side stream of this test's own, created on the HIP runtime the process has loaded and destroyed again at the end.  Not
    one of torch.cuda.Stream()'s: those come from a pool that lives as long as the process, and a pool stream's hardware queue
    is settled when it is first drawn -- drawn here, beside this test's handle, one of the streams that
    tests/test_gpu_overlap.py draws later in the same process shared a queue with another of its lanes (F = 3: 6 overlapping
    pairs of solves instead of 18, the whole suite run twice).  A stream that is gone afterwards leaves the pool as it was."""
    path = next(line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line)
    hip = ctypes.CDLL(path)
    st = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(st), 1) == 0          # hipStreamNonBlocking
    try:
        yield torch.cuda.ExternalStream(st.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(st) == 0


def test_device_tensors_and_capture_read_U_at_replay_time(igt):
    import torch
    case = CC.build((48, 20, 64, 1, 4, False, None))
    B = 8
    dev = lambda a: torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()      # (a copy: the case is read-only)
    pos = [dev(case[k][:B]) for k in ('x0', 'u_prev', 'kparams', 'flags')]
    obs = dev(case['obs'][:B])
    U1, U2 = dev(case['U'][:B]), dev(case['U'][8:8 + B])      # other scenarios' candidates: another answer
    with CC.open_solver(igt, case) as s:
        eager = []
        for Ui in (U1, U2):
            e = s.solve_candidates(*pos, Ui, obs_xy=obs)
            torch.cuda.synchronize()
            eager.append({k: v.cpu().numpy() for k, v in e.items()})
        # against host arrays: the same entry through the staging path
        host = s.solve_candidates(*[case[k][:B] for k in ('x0', 'u_prev', 'kparams', 'flags')], case['U'][:B], obs_xy=case['obs'][:B])
        for k in SOLVE_KEYS:
            assert _same_bytes(host[k], eager[0][k]), k
        U = U1.clone()
        out = {k: torch.empty_like(v) for k, v in e.items()}
        replayed = []
        with _side_stream(torch) as side:
            with torch.cuda.stream(side):
                s.solve_candidates(*pos, U, obs_xy=obs, out=out)      # warm-up on the capture stream
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):                    # a single stream, no parallel branches
                s.solve_candidates(*pos, U, obs_xy=obs, out=out)
            for Ui in (U1, U2):
                U.copy_(Ui)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                replayed.append({k: v.cpu().numpy() for k, v in out.items()})
            del g
    for i in range(2):
        for k in SOLVE_KEYS:
            assert _same_bytes(replayed[i][k], eager[i][k]), (i, k)
    assert (eager[0]['status'] == 0).sum() >= 2
    assert not _same_bytes(replayed[0]['u'], replayed[1]['u']), 'the replay did not read U on the device'


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_and_edges(igt):
    case = CC.build((48, 20, 64, 1, 4, False, None))
    pos, opt = CC.solve_args(case, slice(0, 4))
    U = case['U'][:4]
    with igt.BatchSolver(C=64, dtype='f64', cand_mode='lattice') as s:
        for fn in (s.solve_candidates, s.rollout_candidates):
            with pytest.raises(ValueError, match="cand_mode='table'"):
                fn(*pos, U, **opt)
        # ... and the library itself refuses another family
        n_ptr = len(igt._lib.SYMBOLS['igt_solve_candidates_f64'][1]) - 4
        dummy = np.zeros(8)
        ptrs = [dummy.ctypes.data] * n_ptr
        assert s.lib.igt_solve_candidates_f64(s._h, 1, *ptrs, igt._lib.IGT_MEM_HOST, None) == -1
        assert b'IGT_CAND_TABLE' in s.lib.igt_last_error()
    with igt.BatchSolver(C=64, dtype='f32', cand_mode='table') as s:
        f4 = [p.astype(np.float32) if p.dtype == np.float64 else p for p in pos]
        for fn in (s.solve_candidates, s.rollout_candidates):
            with pytest.raises(ValueError, match="dtype='f64'"):
                fn(*f4, U, obs_xy=opt['obs_xy'].astype(np.float32))
    with igt.BatchSolver(C=64, dtype='f64', cand_mode='table') as s:      # set_candidate_table is never called
        s.set_cinf(*case['cinf'])
        for fn in (s.solve_candidates, s.rollout_candidates):
            for wrong in (U[:3], U[:, :32], U[:, :, :, :19], U[0], None):
                with pytest.raises(ValueError, match=r'U must be \[B,C,2,N\]'):
                    fn(*pos, wrong, **opt)
        assert s.lib.igt_solve_candidates_f64(s._h, 1, *ptrs[:7], None, *ptrs[8:], igt._lib.IGT_MEM_HOST, None) == -1      # null U
        assert b'U is null' in s.lib.igt_last_error()
        assert s.lib.igt_solve_candidates_f64(s._h, -1, *ptrs, igt._lib.IGT_MEM_HOST, None) == -1
        e_pos, e_opt = CC.solve_args(case, slice(0, 0))
        empty = s.solve_candidates(*e_pos, case['U'][:0], **e_opt)
        assert empty['x'].shape == (0, 7, 21) and empty['status'].shape == (0,)
        empty = s.rollout_candidates(*e_pos, case['U'][:0], **e_opt)
        assert empty['cost'].shape == (0, 64)
        got = s.solve_candidates(*pos, U, **opt)                          # works without a shared table ...
        ref = CC.oracle(case)[0][0]
        assert (got['status'] == ref['status'][:4]).all() and (got['argmin'] == ref['argmin'][:4]).all()
        with pytest.raises(igt.IgtError, match='candidate table not set'):      # ... which solve() still asks for
            s.solve(*pos, **opt)
    net = value_net_case(1, 'f64')['net']
    with igt.BatchSolver(C=64, dtype='f64', cand_mode='table', cost_mode='value_net', value_polish_iters=1) as s:
        s.set_value_net(**net)
        b = CC.build((24, 20, 64, 1, 4, False, 3))
        with pytest.raises(TypeError, match='device'):
            s.solve_candidates(b['x0'][:4], b['u_prev'][:4], b['kparams'][:4], b['flags'][:4], b['U'][:4], obs_xy=b['obs'][:4],
                               tv_sv=b['tv_sv'][:4], enc=b['enc'][:4])
