"""Analysis (oracle side, CPU): wave-steps of the float64 lattice search under two mappings of candidates to waves, as a
fraction of 4 N per scenario (four 64-candidate units of N steps each).

  units   today's 64-candidate units of the live rows (unit_layout kind 3), whole-wave early exit: a unit rolls until its
          last candidate has failed;
  pool    one wave per scenario (igt_fast64.h rollout_pool): a lane whose candidate fails or reaches N takes the scenario's
          next candidate number -- one iteration is one control step of every busy lane;
  ideal   alive lane-steps / 64.

How long a candidate holds its lane (`retire`, lives() below):
  'after'   it retires after the step that judged the failing state: |ey| of state k is judged by step k, so k + 1 steps; the
            collision of state k is folded in by step k and seen by step k + 1, so k + 2 steps (collision_lag; without it
            the collision counts like |ey|, which is what this tool said before and undercounts);
  'early'   rollout_pool today: at the end of a step the lane tests the state it reached and the collision of the state it left,
            so k steps for |ey| of state k (one at the least) and k + 1 for a collision of state k.
Step counts only: the refill bookkeeping costs instructions on top, and the sub-step votes see lanes at different k.
    python tools/refill_model.py [B] [seed]            both settings and their ratio
    python tools/refill_model.py --votes [B] [seed]    which sub-step variant each wave-step votes (votes() below), both settings
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from death_steps import first_failures     # noqa: E402


def live_rows(B, P, sc, G):
    """Rows whose (a, v) recurrence holds the speed box (the terminal set is left out: a row mask close to accel_rows_kernel's)."""
    from oracle import np_oracle as O
    U = O.candidates_lattice(sc['u_prev'], P, G * G)[:, ::G]          # one candidate per row: [B, G, 2, N]
    v = sc['x0'][:, 5:6, None] + np.concatenate([np.zeros((B, G, 1)), np.cumsum(P.dt * U[:, :, 0, :], -1)], -1)
    return ~(np.maximum(P.v_min - v[..., :P.N], v[..., :P.N] - P.v_max) > P.feas_tol).any(-1)


def numbering(G, rows):
    """candidate indices in unit_candidate's live-row order: columns from the centre outwards, live rows within a column"""
    cols = [G // 2 + (r >> 1) if r % 2 == 0 else G // 2 - 1 - (r >> 1) for r in range(G)]
    return np.array([i * G + j for j in cols for i in np.flatnonzero(rows)], dtype=np.int64)


def lives(first, N, retire='early', collision_lag=True):
    """control steps a candidate rolls before its lane is free, from first_failures()'s per-verdict states"""
    state = np.minimum(first['v'], first['ey'])                       # verdicts step_head folds in for its own state
    if retire == 'early':
        return np.minimum(np.maximum(np.minimum(state, first['col'] + 1), 1), N)
    assert retire == 'after', retire
    return np.minimum(np.minimum(state + 1, first['col'] + (2 if collision_lag else 1)), N)


def pool_steps(B=512, seed=0, N=20, C=256, retire='early', collision_lag=True):
    """wave-steps of the pool per scenario, [B] (0: no live row)"""
    first, P = first_failures(B, N, C, seed)
    return _walk(B, seed, N, C, lives(first, N, retire, collision_lag), P)['pool_per_scenario']


def _walk(B, seed, N, C, life_all, P, life_unit=None):
    from igtmpc.scenarios import make_batch
    G = int(round(C ** 0.5))
    sc = make_batch(B, N, P.dt, seed=seed, dtype=np.float64)
    live = live_rows(B, P, sc, G)
    unit_steps = pool_steps = ideal = 0.0
    refill_iters = iters = 0
    per = np.zeros(B, dtype=np.int64)
    for b in range(B):
        idx = numbering(G, live[b])
        if idx.size == 0:
            continue
        life = life_all[b, idx]                                       # steps a candidate rolls before it retires
        lu = life if life_unit is None else life_unit[b, idx]
        for u in range(0, idx.size, 64):                              # units: until the last lane leaves
            unit_steps += lu[u:u + 64].max()
        ideal += life.sum() / 64.0
        lanes = np.zeros(64, dtype=np.int64)                          # steps left per lane
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
            per[b] += 1
            iters += 1
    norm = 4.0 * N * B
    return dict(units=unit_steps / norm, pool=pool_steps / norm, ideal=ideal / norm,
                iterations_with_refill=refill_iters / max(iters, 1), pool_per_scenario=per)


def model(B=512, seed=0, N=20, C=256, retire='early', collision_lag=True):
    """units: always with the lives of 'after' without the lag -- a unit leaves through step_head's vote, which this tool counted so"""
    first, P = first_failures(B, N, C, seed)
    r = _walk(B, seed, N, C, lives(first, N, retire, collision_lag), P, lives(first, N, 'after', False))
    del r['pool_per_scenario']
    return r


def votes(B=256, seed=0, N=20, C=256, retire='early', collision_lag=True):
    """The sub-step variant a wave votes at every wave-step of the two mappings, with substeps()'s whole-step vote
    (igt_fast64.h): `clear` -- every busy lane's step stays off the arc, K = 0 throughout; `inside` -- every lane's stays on it,
    K = k_v; else the per-sub-step fallback.  A unit's lanes vote until the unit leaves (dead lanes roll on); a pool's busy
    lanes vote each at its own k, for as long as lives() says (the units' lives are always those of 'after', without the lag:
    a unit leaves through step_head's vote).  -> shares (clear, inside, fallback) of the wave-steps, for units and pool."""
    from oracle import np_oracle as O
    from igtmpc.scenarios import make_batch
    first, P = first_failures(B, N, C, seed)
    life_pool, life_unit = lives(first, N, retire, collision_lag), lives(first, N, 'after', False)
    G = int(round(C ** 0.5))
    sc = make_batch(B, N, P.dt, seed=seed, dtype=np.float64)
    X = O.rollout_frenet(O.apply_flags(sc['x0'], sc['flags'])[:, None, :], O.candidates_lattice(sc['u_prev'], P, C),
                         sc['kparams'][:, None, :], P)
    b0, b1, kv = (sc['kparams'][:, i, None, None] for i in range(3))
    s, v, ey = X[..., O.IS, :N], X[..., O.IV, :N], X[..., O.IEY, :N]
    a = O.candidates_lattice(sc['u_prev'], P, C)[:, :, 0, :]
    m = (2 * P.dt) * (np.abs(v) + P.dt * np.abs(a))                      # reach of one control step
    clear = ((s - b0) + m < 0) | ((s - b1) - m > 0) | (kv == 0)
    inside = ((s - b0) - m > 0) & ((s - b1) + m < 0) & (np.abs(kv) * (np.abs(ey) + 0.5 * m) < 0.5)
    cls = np.where(clear, 0, np.where(inside, 1, 2))                     # [B, C, N]
    vote = lambda c: 0 if (c == 0).all() else 1 if (c == 1).all() else 2
    live = live_rows(B, P, sc, G)
    mix = {'units': np.zeros(3), 'pool': np.zeros(3)}
    for b in range(B):
        idx = numbering(G, live[b])
        if idx.size == 0:
            continue
        life = life_pool[b, idx]
        for u in range(0, idx.size, 64):
            for k in range(life_unit[b, idx[u:u + 64]].max()):
                mix['units'][vote(cls[b, idx[u:u + 64], k])] += 1
        lanes = np.zeros(64, dtype=np.int64)
        cand = np.zeros(64, dtype=np.int64)
        kk = np.zeros(64, dtype=np.int64)
        nxt = 0
        while True:
            idle = lanes == 0
            take = min(int(idle.sum()), idx.size - nxt)
            if take > 0:
                w = np.flatnonzero(idle)[:take]
                lanes[w], cand[w], kk[w] = life[nxt:nxt + take], idx[nxt:nxt + take], 0
                nxt += take
            act = lanes > 0
            if not act.any():
                break
            mix['pool'][vote(cls[b, cand[act], kk[act]])] += 1
            lanes[act] -= 1
            kk[act] += 1
    return {k: v / v.sum() for k, v in mix.items()}


SETTINGS = (('after its step', dict(retire='after', collision_lag=True)),
            ('at the end of the step before', dict(retire='early')))

if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--votes':
        a = sys.argv[2:]
        for name, kw in SETTINGS:
            r = votes(int(a[0]) if a else 256, int(a[1]) if len(a) > 1 else 0, **kw)
            print(f'a failed candidate retires {name}:')
            for k in ('units', 'pool'):
                print(f'  {k:5s}: K = 0 on {r[k][0]:.1%} of the wave-steps, K = k_v on {r[k][1]:.1%}, '
                      f'per-sub-step fallback on {r[k][2]:.1%}')
        sys.exit(0)
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    res = []
    for name, kw in SETTINGS:
        r = model(B, seed, **kw)
        res.append(r)
        print(f'B = {B}, a failed candidate retires {name}: wave-steps / (4 N B): units {r["units"]:.4f}  pool {r["pool"]:.4f} '
              f'({r["pool"] / r["units"] - 1:+.1%})  ideal {r["ideal"]:.4f};  iterations that refill {r["iterations_with_refill"]:.2f}')
    print(f'pool, early / after: {res[1]["pool"] / res[0]["pool"] - 1:+.1%}')
