"""The polish of the winner (igtmpc.h polish_iters; csrc/igt_kernels_f64.hip polish_f64_kernel) restated in numpy on the
oracle's functions (np_oracle.rollout_frenet, stage_cost, constraint_violation, apply_flags) -- tests only.

Per solved scenario, from the winner u [2, N] with cost J0, `iters` times:
  1. gradient: g_c = (J(u + eps e_c) - J0) / eps over the 2 N inputs, eps = 1e-4 (component c = row c // N, step c % N),
     no projection, no verdicts; a non-finite J gives 0;
  2. direction: d = -g / scale, scale = max(max|g_a| / (4 dt jerk), max|g_df| / (4 dt steer_rate)) + 1e-30 (steer_rate = 0: the
     steering row of d is 0 and its term is left out);
  3. line search: 64 trials project(u + 2^(-m/3) d) -- step k clamped to the rate window around the projected step k - 1
     (u_prev for k = 0), then to the input box --, each judged by every verdict, the rate verdict included; the feasible trial
     of least cost, ties to the lowest m;
  4. accepted only if strictly cheaper than J0, else the scenario stops.
All scenarios are carried side by side (arrays [n, ...]); a scenario that stopped is left alone."""
import numpy as np

import np_oracle as O

EPS = 1e-4
TRIALS = 64


def project(U, u_prev, P):
    """sequential clamp to the rate limits and the box; U [..., 2, N], u_prev [..., 2] broadcastable to U's leading axes"""
    N = U.shape[-1]
    ra, rd = P.dt * P.jerk, P.dt * P.steer_rate
    out = np.empty_like(U)
    pa = np.broadcast_to(u_prev[..., 0], U.shape[:-2]).copy()
    pd = np.broadcast_to(u_prev[..., 1], U.shape[:-2]).copy()
    for k in range(N):
        a = np.clip(np.clip(U[..., 0, k], pa - ra, pa + ra), P.a_min, P.a_max)
        d = np.clip(np.clip(U[..., 1, k], pd - rd, pd + rd), -P.df_max, P.df_max)
        out[..., 0, k] = a
        out[..., 1, k] = d
        pa, pd = a, d
    return out


def evaluate(batch, idx, U, P, cinf):
    """cost, feasibility and worst verdict margin of U [n, m, 2, N] for the scenarios idx [n] of the batch"""
    f = lambda k: np.asarray(batch[k], dtype=np.float64)[idx]
    x0 = O.apply_flags(f('x0'), np.asarray(batch['flags'])[idx])
    X = O.rollout_frenet(x0[:, None, :], U, f('kparams')[:, None, :], P)
    J = O.stage_cost(X, U, P)
    A, b = (None, None) if cinf is None else cinf
    g, mask = O.constraint_violation(X, U, f('u_prev')[:, None, :], f('obs_xy')[:, None], A, b, P, check_rate=True)
    return J, (mask == 0) & np.isfinite(J), g


def polish(batch, idx, u, J0, iters, P, cinf, noise=0.0, rng=None):
    """-> list over it = 0 .. iters of (u [n, 2, N], J [n]) -- entry 0 is the seed --, and per iteration the gap between the two
    cheapest feasible trials (inf where there are fewer than two): what the tie set-aside of the device comparison reads.
    noise: standard deviation of a perturbation of the gradient (how far rounding of the gradient can move the answer)."""
    idx = np.asarray(idx)
    u = np.array(u, dtype=np.float64, copy=True)
    J0 = np.array(J0, dtype=np.float64, copy=True)
    n, _, N = u.shape
    ra, rd = P.dt * P.jerk, P.dt * P.steer_rate
    u_prev = np.asarray(batch['u_prev'], dtype=np.float64)[idx]
    alive = np.ones(n, dtype=bool)
    hist, ties = [(u.copy(), J0.copy())], []
    al = 2.0 ** (-np.arange(TRIALS) / 3.0)
    for _ in range(iters):
        Up = np.repeat(u[:, None], 2 * N, axis=1)                       # [n, 2N, 2, N]
        for c in range(2 * N):
            Up[:, c, c // N, c % N] += EPS
        Jp, _, _ = evaluate(batch, idx, Up, P, cinf)
        with np.errstate(invalid='ignore'):
            g = np.where(np.isfinite(Jp), (Jp - J0[:, None]) / EPS, 0.0).reshape(n, 2, N)
        if noise:
            g = g + noise * rng.standard_normal(g.shape)
        ma, md = np.abs(g[:, 0]).max(axis=-1), np.abs(g[:, 1]).max(axis=-1)
        scale = (np.maximum(ma / (4 * ra), md / (4 * rd)) if rd > 0 else ma / (4 * ra)) + 1e-30
        d = -g / scale[:, None, None]
        if not rd > 0:
            d[:, 1] = 0.0
        Uc = project(u[:, None] + al[None, :, None, None] * d[:, None], u_prev[:, None, :], P)
        Jc, fc, _ = evaluate(batch, idx, Uc, P, cinf)
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
