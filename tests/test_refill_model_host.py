"""CPU: tools/refill_model.py counts the wave-steps of the pooled lattice search under two rules for how long a failed candidate
holds its lane -- 'after' its step (the loop before early retirement; with collision_lag the collision of state k costs k + 2
steps, as that loop did) and 'early' (igt_fast64.h rollout_pool: tested at the end of the step that reached the state).
On 64 seeded scenarios: a candidate never lives longer under 'early', no scenario takes more wave-steps, the total is strictly
smaller; and 'after' without the lag is the tool's earlier count, restated here from death_steps().
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

B, SEED, N, C = 64, 11, 20, 256


@pytest.fixture(scope='module')
def rm():
    import refill_model
    return refill_model


@pytest.fixture(scope='module')
def first():
    from death_steps import first_failures
    return first_failures(B, N, C, SEED)[0]


def test_lives_early_never_longer(rm, first):
    after = rm.lives(first, N, 'after', True)
    early = rm.lives(first, N, 'early')
    legacy = rm.lives(first, N, 'after', False)
    assert early.min() >= 1 and after.max() <= N
    assert (early <= legacy).all() and (legacy <= after).all()
    saves = (after < N) & (first['ey'] > 0)          # retired before the horizon's end, not at state 0: one step saved at the least
    assert saves.any() and (early[saves] < after[saves]).all()
    # a collision of state k: k + 2 steps after, k + 1 early; |ey| of state k: k + 1 after, k early
    one = {k: np.array([[v]]) for k, v in (('v', N + 1), ('ey', N + 1), ('col', 5))}
    assert (rm.lives(one, N, 'after', True)[0, 0], rm.lives(one, N, 'after', False)[0, 0], rm.lives(one, N, 'early')[0, 0]) == (7, 6, 6)
    one = {k: np.array([[v]]) for k, v in (('v', N + 1), ('ey', 5), ('col', N + 1))}
    assert (rm.lives(one, N, 'after', True)[0, 0], rm.lives(one, N, 'early')[0, 0]) == (6, 5)
    one = {k: np.array([[v]]) for k, v in (('v', N + 1), ('ey', 0), ('col', N + 1))}      # state 0 fails: still one step
    assert (rm.lives(one, N, 'after', True)[0, 0], rm.lives(one, N, 'early')[0, 0]) == (1, 1)
    one = {k: np.array([[v]]) for k, v in (('v', N + 1), ('ey', N + 1), ('col', N + 1))}  # survivor
    assert (rm.lives(one, N, 'after', True)[0, 0], rm.lives(one, N, 'early')[0, 0]) == (N, N)


def test_early_takes_no_more_wave_steps(rm):
    after = rm.pool_steps(B, SEED, N, C, retire='after', collision_lag=True)
    early = rm.pool_steps(B, SEED, N, C, retire='early')
    print(f'wave-steps: after {after.sum()}, early {early.sum()} ({early.sum() / after.sum() - 1:+.1%})')
    assert after.shape == early.shape == (B,)
    assert (after > 0).sum() > B // 2, 'most scenarios have a live row'
    assert (early <= after).all()
    assert early.sum() < after.sum()


def _model_before(B, seed, N, C):
    """model() as it was before the retirement settings: life = min(dead + 1, N) for units and pool alike"""
    from death_steps import death_steps
    from igtmpc.scenarios import make_batch
    import refill_model as R
    dead, P = death_steps(B, N, C, seed)
    G = int(round(C ** 0.5))
    sc = make_batch(B, N, P.dt, seed=seed, dtype=np.float64)
    live = R.live_rows(B, P, sc, G)
    unit_steps = pool_steps = ideal = 0.0
    refill_iters = iters = 0
    for b in range(B):
        idx = R.numbering(G, live[b])
        if idx.size == 0:
            continue
        life = np.minimum(dead[b, idx] + 1, N)
        for u in range(0, idx.size, 64):
            unit_steps += life[u:u + 64].max()
        ideal += life.sum() / 64.0
        lanes = np.zeros(64, dtype=np.int64)
        nxt = 0
        while True:
            idle = lanes == 0
            take = min(int(idle.sum()), idx.size - nxt)
            if take > 0:
                lanes[np.flatnonzero(idle)[:take]] = life[nxt:nxt + take]
                nxt += take
                refill_iters += 1
            if not (lanes > 0).any():
                break
            lanes[lanes > 0] -= 1
            pool_steps += 1
            iters += 1
    norm = 4.0 * N * B
    return dict(units=unit_steps / norm, pool=pool_steps / norm, ideal=ideal / norm,
                iterations_with_refill=refill_iters / max(iters, 1))


def test_after_without_lag_is_the_earlier_count(rm):
    assert rm.model(B, SEED, N, C, retire='after', collision_lag=False) == _model_before(B, SEED, N, C)
