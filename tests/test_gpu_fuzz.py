"""-m gpu : randomised configurations of the float64 entry points against the numpy oracle.

The other parity tests run the reference's configuration (N = 20 or 40, 256 candidates, 4 RK4 sub-steps, dt = 0.1) at
many batch sizes; the kernels, however, are templates over much more than that -- the build for any n_rk4 next to the one
for 4, high-order offset polynomials for coarse discretisations, 1 to 64 units per scenario, steering tables that fit LDS
or do not, one or more obstacles, trajectories kept by the search pass or re-rolled, one wave per unit or queues.  Here a
seeded generator draws the configuration -- horizon, discretisation, dt, candidate count, family, refinement passes,
obstacle count, limits, batch size -- and every draw must give the oracle's answer: status and arg-min exactly wherever
the decision is not inside 1e-9 of a threshold, tie or break-point, trajectories and costs to 1e-9."""
import numpy as np
import pytest

import np_oracle as O
from helpers import rel_err
from parity_cases import FUZZ_EXT_F32_SEEDS as EXT_F32_SEEDS, FUZZ_EXT_SEEDS as EXT_SEEDS, FUZZ_F32_SEEDS as F32_SEEDS, \
    FUZZ_N_SEEDS as N_SEEDS, fuzz_case, fuzz_draw as _draw


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_random_configuration_matches_oracle(seed, golden_dir):
    _run(seed, golden_dir, 'f64')


@pytest.mark.gpu
@pytest.mark.parametrize('seed', F32_SEEDS)
def test_random_configuration_matches_oracle_f32(seed, golden_dir):
    """The float32 entry points on the same kind of draws, at BASELINE.json's 1e-5 with the float32 set-asides of
    test_gpu_parity.py (threshold / break-point within 1e-7, near-ties; value network: 2e-5)."""
    _run(seed, golden_dir, 'f32')


@pytest.mark.gpu
@pytest.mark.parametrize('seed', EXT_SEEDS)
def test_random_configuration_at_the_advertised_limits_matches_oracle(seed, golden_dir):
    _run(seed, golden_dir, 'f64')


@pytest.mark.gpu
@pytest.mark.parametrize('seed', EXT_F32_SEEDS)
def test_random_configuration_at_the_advertised_limits_matches_oracle_f32(seed, golden_dir):
    _run(seed, golden_dir, 'f32')


def _run(seed, golden_dir, dtype):
    import igtmpc
    from parity_cases import check_case, device_solve, open_solver, oracle_passes, solve_args
    case = fuzz_case(seed, dtype)
    cfg, B, P = case['cfg'], case['B'], case['P']
    f32 = dtype == 'f32'
    tol, utol, eps = case['tol'], case['utol'], case['eps']
    with open_solver(igtmpc, case) as s:
        got = device_solve(s, case)
        n_all = min(B, 4)
        pos, kw = solve_args(case, n_all)
        allc = s.rollout_all(*pos, **kw)
    oracle = oracle_passes(case)
    passes, x0, kp = oracle
    first = passes[0]
    # every candidate of the first pass: controls, trajectories, verdicts (the refinement passes re-centre on a winner)
    if cfg['refine'] == 0:
        bp_all = O.breakpoint_distance(x0[:n_all], first['U'][:n_all], kp[:n_all], P)
        clear = bp_all > eps
        if f32:     # float32 error grows with the excursion: only roll-outs that stay near the lane are held to 1e-5 (every
                    # feasible one does: |e_y| <= ey_lim)
            clear &= (np.abs(first['X'][:n_all, :, 3, :]).max(axis=-1) <= 1.0) & (np.abs(first['X'][:n_all, :, 4, :]).max(axis=-1) <= 0.5)
        if not clear.any():
            clear[...] = False
        assert clear.sum() == 0 or rel_err(allc['U'][clear], first['U'][:n_all][clear]).max() <= utol, cfg
        # ... those that stay clear of the model's singularity 1 - K e_y = 0 (frenet.py:73): a wild candidate of a long horizon
        # drifts tens of metres off the lane, and next to the pole rounding differences are amplified without bound
        # (seed 31: min |1 - K e_y| = 2.7e-4, 0.25 relative).  Every FEASIBLE candidate has |e_y| <= ey_lim and is compared.
        pole = np.abs(1.0 - kp[:n_all, :, 2:3] * first['X'][:n_all, :, 3, :]).min(axis=-1) > 0.1
        fin = clear & pole & np.isfinite(first['X'][:n_all]).all(axis=(-1, -2))
        assert (first['feas'][:n_all] <= pole).all()
        assert fin.sum() == 0 or rel_err(allc['X'][fin], first['X'][:n_all][fin]).max() <= tol, cfg
        thr = fin & (np.abs(first['g'][:n_all] - P.feas_tol) > (1e-6 if f32 else 1e-9))
        assert ((allc['viol'] == 0) == first['feas'][:n_all])[thr].all(), cfg
    # the solve: a scenario is set aside when ANY pass decided it inside 1e-9 (a different winner re-centres the next pass)
    check_case(case, got, oracle)


def test_the_draws_cover_the_template_space():
    """The seeds above are only worth something if they reach the corners: both RK4 builds, coarse and fine steps,
    1 / 4 / 16 units per scenario, every family, refinement, warm starts, 0 / 1 / 2 obstacles, with and without the terminal
    set, both value-network architectures, batches either side of the kept-trajectory bound (units <= 1024 SIMDs)."""
    cfgs = [_draw(s) for s in range(N_SEEDS)]
    assert {c['net'] for c in cfgs} == {0, 1, 3} and any(c['warm'] for c in cfgs)
    assert any(c['net'] and c['cand'] == 'track' for c in cfgs) and any(c['net'] and c['refine'] for c in cfgs)
    assert any(c['B'] * c['C'] // 64 > 1024 for c in cfgs) and any(c['B'] * c['C'] // 64 <= 1024 and c['B'] > 8 for c in cfgs)
    f32 = [_draw(s) for s in F32_SEEDS]
    assert {c['cand'] for c in f32} == {'lattice', 'ramp_hold', 'track'} and any(c['net'] for c in f32) and any(c['warm'] for c in f32)
    assert {c['C'] for c in f32} == {64, 256, 1024} and any(c['n_rk4'] != 4 for c in f32) and any(c['refine'] for c in f32)
    assert {c['n_rk4'] == 4 for c in cfgs} == {True, False}
    assert {c['C'] for c in cfgs} == {64, 256, 1024}
    assert {c['cand'] for c in cfgs} == {'lattice', 'ramp_hold', 'track'}
    assert {c['n_obs'] for c in cfgs} == {0, 1, 2}
    assert {c['terminal'] for c in cfgs} == {True, False}
    assert any(c['refine'] > 0 for c in cfgs) and any(c['N'] > 20 for c in cfgs) and any(c['N'] < 12 for c in cfgs)
    assert any(c['n_rk4'] <= 2 and c['dt'] >= 0.1 for c in cfgs)          # the high-order offset polynomials
    assert any(c['B'] == 1 for c in cfgs) and any(c['B'] >= 17 for c in cfgs)
    ext = [_draw(s) for s in list(EXT_SEEDS) + list(EXT_F32_SEEDS)]
    assert {c['n_obs'] for c in ext} == {2, 3, 4} and {c['N'] for c in ext} == {48, 64} and {c['C'] for c in ext} == {64, 256}
    assert any(c['N'] == 64 and c['C'] == 64 for c in ext) and any(c['N'] == 64 and c['C'] == 256 for c in ext)     # table fits / does not
    assert any(c['B'] * c['C'] // 64 > 4096 for c in ext) and {c['cand'] for c in ext} == {'lattice', 'ramp_hold', 'track'}
    assert any(c['n_obs'] == 4 and c['N'] == 64 for c in ext)
