"""The polish of the winner under the value-network cost (gt_mpc) restated in numpy on the oracle's functions and the restatements
it is built from -- tests only.  It is the adjoint mode of the progress-cost polish (adjoint_restated.polish_adjoint) with the
terminal term exchanged; the device does not have it yet (`polish_iters > 0` stays refused with IGT_COST_VALUE_NET), and this is
the statement a device implementation is compared against.

J(u) = sum_{k<=N} (epsi_k^2 + ey_k^2) + w_u sum_{k<N} (a_k^2 + df_k^2) - V_out(s_N, v_N) (mpc.py:356-369).  Per solved scenario,
from the winner u [2, N] with cost J0, `iters` times:
  1. gradient: value_gradient_restated.cost_gradient_vn at the plan -- the costate recursion from the terminal seed
     (-dV_out/ds_N, 2 ey_N, 2 epsi_N, -dV_out/dv_N), the partials at the plan's own (s_N, v_N); non-finite entries 0;
  2. direction: d = -g / scale, scale = max(max|g_a| / (4 dt jerk), max|g_df| / (4 dt steer_rate)) + 1e-30 (steer_rate = 0: the
     steering row of d is 0 and its term is left out);
  3. trials: 64 of them, polish_restated.project(u + 2^(-m/3) d), each judged by every verdict, the rate verdict included; a
     trial's cost is np_oracle.stage_cost with np_oracle.terminal_value of its own terminal state -- no progress term;
  4. the feasible trial of least cost, ties to the lowest m, accepted only if strictly cheaper than J0, else the scenario stops.
All scenarios are carried side by side (arrays [n, ...]); a scenario that stopped is left alone."""
import numpy as np

import np_oracle as O
import polish_restated as R
import value_gradient_restated as VG


def evaluate(batch, idx, U, P, cinf, net):
    """cost under the value network, feasibility and worst verdict margin of U [n, m, 2, N] for the scenarios idx [n]"""
    f = lambda k: np.asarray(batch[k], dtype=np.float64)[idx]
    N = U.shape[-1]
    x0 = O.apply_flags(f('x0'), np.asarray(batch['flags'])[idx])
    X = O.rollout_frenet(x0[:, None, :], U, f('kparams')[:, None, :], P)
    V = O.terminal_value(net, X[..., O.IS, N], X[..., O.IV, N], f('tv_sv'), f('enc'))
    J = O.stage_cost(X, U, P, terminal_value=V)
    A, b = (None, None) if cinf is None else cinf
    g, mask = O.constraint_violation(X, U, f('u_prev')[:, None, :], f('obs_xy')[:, None], A, b, P, check_rate=True)
    return J, (mask == 0) & np.isfinite(J), g


def polish_value(batch, idx, u, J0, iters, P, cinf, net):
    """-> (hist, ties) as adjoint_restated.polish_adjoint: hist is the list over it = 0 .. iters of (u [n, 2, N], J [n]) --
    entry 0 is the seed --, ties per iteration the gap between the two cheapest feasible trials (inf where fewer than two)."""
    idx = np.asarray(idx)
    u = np.array(u, dtype=np.float64, copy=True)
    J0 = np.array(J0, dtype=np.float64, copy=True)
    n, _, N = u.shape
    ra, rd = P.dt * P.jerk, P.dt * P.steer_rate
    f = lambda k: np.asarray(batch[k], dtype=np.float64)[idx]
    u_prev = f('u_prev')
    alive = np.ones(n, dtype=bool)
    hist, ties = [(u.copy(), J0.copy())], []
    al = 2.0 ** (-np.arange(R.TRIALS) / 3.0)
    for _ in range(iters):
        _, g = VG.cost_gradient_vn(f('x0'), f('kparams'), np.asarray(batch['flags'])[idx], f('tv_sv'), f('enc'), u, P, net)
        g = np.where(np.isfinite(g), g, 0.0)
        ma, md = np.abs(g[:, 0]).max(axis=-1), np.abs(g[:, 1]).max(axis=-1)
        scale = (np.maximum(ma / (4 * ra), md / (4 * rd)) if rd > 0 else ma / (4 * ra)) + 1e-30
        d = -g / scale[:, None, None]
        if not rd > 0:
            d[:, 1] = 0.0
        Uc = R.project(u[:, None] + al[None, :, None, None] * d[:, None], u_prev[:, None, :], P)
        Jc, fc, _ = evaluate(batch, idx, Uc, P, cinf, net)
        Jc = np.where(fc, Jc, np.inf)
        m = Jc.argmin(axis=1)                                           # first minimum: the lowest m
        Jm = Jc[np.arange(n), m]
        two = np.sort(Jc, axis=1)[:, :2]
        with np.errstate(invalid='ignore'):
            ties.append(np.where(np.isfinite(two[:, 1]), two[:, 1] - two[:, 0], np.inf))
        take = alive & (Jm < J0)
        u = np.where(take[:, None, None], Uc[np.arange(n), m], u)
        J0 = np.where(take, Jm, J0)
        alive = take
        hist.append((u.copy(), J0.copy()))
    return hist, ties
