"""Analysis (oracle side, CPU): wave-steps of the float64 lattice search under two mappings of candidates to waves, as a
fraction of 4 N per scenario (four 64-candidate units of N steps each).

  units   today's 64-candidate units of the live rows (unit_layout kind 3), whole-wave early exit: a unit rolls until its
          last candidate has failed;
  pool    one wave per scenario (igt_fast64.h rollout_pool): a lane whose candidate fails or reaches N takes the scenario's
          next candidate number -- one iteration is one control step of every busy lane;
  ideal   alive lane-steps / 64.

A candidate that fails a verdict of state k has rolled k + 1 steps in the pool roll-out (it retires after its step).
Step counts only: the refill bookkeeping costs instructions on top, and the sub-step votes see lanes at different k.
    python tools/refill_model.py [B] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from death_steps import death_steps        # noqa: E402


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


def model(B=512, seed=0, N=20, C=256):
    from oracle import np_oracle as O
    from igtmpc.scenarios import make_batch
    dead, P = death_steps(B, N, C, seed)
    G = int(round(C ** 0.5))
    sc = make_batch(B, N, P.dt, seed=seed, dtype=np.float64)
    live = live_rows(B, P, sc, G)
    unit_steps = pool_steps = ideal = 0.0
    refill_iters = iters = 0
    for b in range(B):
        idx = numbering(G, live[b])
        if idx.size == 0:
            continue
        life = np.minimum(dead[b, idx] + 1, N)                        # steps a candidate rolls before it retires
        for u in range(0, idx.size, 64):                              # units: until the last lane leaves
            unit_steps += life[u:u + 64].max()
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
            iters += 1
    norm = 4.0 * N * B
    return dict(units=unit_steps / norm, pool=pool_steps / norm, ideal=ideal / norm,
                iterations_with_refill=refill_iters / max(iters, 1))


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    r = model(B, seed)
    print(f'B = {B}: wave-steps / (4 N B): units {r["units"]:.3f}  pool {r["pool"]:.3f} ({r["pool"] / r["units"] - 1:+.1%})  '
          f'ideal {r["ideal"]:.3f};  iterations that refill {r["iterations_with_refill"]:.2f}')
