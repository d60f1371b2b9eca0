"""The analytic gradient of the progress cost (igtmpc.h igt_cost_gradient_f64; csrc/igt_adjoint64.h) and the adjoint mode of the
polish (igt_set_polish_gradient) restated in numpy on the oracle's model (np_oracle.frenet_rk4_step, stage_cost) -- tests only.

J(u) = sum_{k<=N} (epsi_k^2 + ey_k^2) + w_u sum_{k<N} (a_k^2 + df_k^2) - (s_N - s_0) over the RK4 roll-out from x0.  The cost reads
(s, ey, epsi) and u only, s feeds back through the piecewise-constant K(s) alone (taken as locally constant: d x_k+1 / d s_k is the
unit column) and v_k+1 = v_k + dt a_k, so one control step's Jacobian is five tangent directions (ey, epsi, v, a, df) over the
rows (s, ey, epsi), carried in forward mode through the stages of np_oracle._deriv (step_jacobian); the costate recursion
lam_k = A_k^T lam_k+1 + q_k then runs backwards over the nodes of np_oracle.rollout_frenet (cost_gradient).

polish_adjoint is polish_restated.polish with step 1 replaced: g is this gradient at the current plan (non-finite entries 0);
steps 2-4 -- direction scaling, the 64 projected trials judged by every verdict, acceptance only when strictly cheaper -- are the
same statements on the same helpers (project, evaluate)."""
import numpy as np

import np_oracle as O
import polish_restated as R


def step_jacobian(x, a, df, kp, P):
    """x[..., 7] (planner order), a[...], df[...], kp[..., 3] -> T[..., 3, 5]: rows (s, ey, epsi) of x_k+1, columns
    d / d (ey, epsi, v) of x_k and d / d (a_k, df_k); K(s) locally constant."""
    x, a, df = (np.asarray(q, dtype=np.float64) for q in (x, a, df))
    r = P.l_r / (P.l_f + P.l_r)
    h = P.dt / P.n_rk4
    beta = np.arctan(r * np.tan(df))
    dbeta = r / (np.cos(df) ** 2 + (r * np.sin(df)) ** 2)
    sinb, cosb = np.sin(beta), np.cos(beta)
    s, ey, ep, v = x[..., O.IS], x[..., O.IEY], x[..., O.IEPSI], x[..., O.IV]
    shape = np.broadcast_shapes(s.shape, a.shape)
    T = np.zeros(shape + (3, 5))
    T[..., 1, 0] = 1.0
    T[..., 2, 1] = 1.0
    tb = np.zeros(shape + (5,))
    tb[..., 4] = dbeta                                      # d beta in each direction

    def stage(s_, ey_, ep_, v_, Ta, tv):
        """derivative rows (s, ey, epsi) at the stage argument and their tangents [..., 3, 5] for argument tangents Ta, tv"""
        K = O.curvature(s_, kp)
        D = 1.0 / (1.0 - K * ey_)
        sn, cs = np.sin(beta + ep_), np.cos(beta + ep_)
        ks = v_ * cs * D
        ke = v_ * sn
        kp_ = v_ * sinb / P.l_r - ks * K
        th = Ta[..., 2, :] + tb                             # tangent of beta + epsi
        ts = (ks * D * K)[..., None] * Ta[..., 1, :] - (v_ * sn * D)[..., None] * th + (cs * D)[..., None] * tv
        te = (v_ * cs)[..., None] * th + sn[..., None] * tv
        tp = (sinb / P.l_r)[..., None] * tv + (v_ * cosb / P.l_r)[..., None] * tb - K[..., None] * ts
        return (ks, ke, kp_), np.stack([ts, te, tp], axis=-2)

    one = np.ones(shape)
    for j in range(P.n_rk4):
        tv0 = np.zeros(shape + (5,))
        tv0[..., 2] = 1.0
        acc, accT = None, None
        k, kT = (0.0, 0.0, 0.0), 0.0
        for c, w in ((0.0, 1.0), (h / 2, 2.0), (h / 2, 2.0), (h, 1.0)):
            tv = tv0.copy()
            tv[..., 3] = j * h + c                          # d v / d a at this stage
            k, kT = stage(s + c * k[0], ey + c * k[1], ep + c * k[2], (v + c * a) * one, T + c * kT, tv)
            acc = [w * q for q in k] if acc is None else [p + w * q for p, q in zip(acc, k)]
            accT = w * kT if accT is None else accT + w * kT
        s, ey, ep = s + h / 6 * acc[0], ey + h / 6 * acc[1], ep + h / 6 * acc[2]
        v = v + h * a
        T = T + h / 6 * accT
    return T


def cost_gradient(x0, kp, flags, U, P):
    """x0[B,7] kp[B,3] flags[B] U[B,2,N] -> (J[B], g[B,2,N]): the progress cost of np_oracle.stage_cost over rollout_frenet and
    its gradient by every a_k, df_k -- no projection, no verdicts; a non-finite cost gives a NaN row."""
    x0 = O.apply_flags(np.asarray(x0, dtype=np.float64), flags)
    U = np.asarray(U, dtype=np.float64)
    kp = np.asarray(kp, dtype=np.float64)
    N = U.shape[-1]
    with np.errstate(all='ignore'):
        X = O.rollout_frenet(x0, U, kp, P)
        J = O.stage_cost(X, U, P)
        g = np.empty_like(U)
        lam = np.stack([-np.ones_like(J), 2 * X[..., O.IEY, N], 2 * X[..., O.IEPSI, N], np.zeros_like(J)], axis=-1)
        for k in range(N - 1, -1, -1):
            T = step_jacobian(X[..., :, k], U[..., 0, k], U[..., 1, k], kp, P)
            c = np.einsum('...rd,...r->...d', T, lam[..., :3])
            g[..., 0, k] = 2 * P.w_u * U[..., 0, k] + c[..., 3] + P.dt * lam[..., 3]
            g[..., 1, k] = 2 * P.w_u * U[..., 1, k] + c[..., 4]
            lam = np.stack([lam[..., 0], 2 * X[..., O.IEY, k] + c[..., 0], 2 * X[..., O.IEPSI, k] + c[..., 1],
                            lam[..., 3] + c[..., 2]], axis=-1)
    g[~np.isfinite(J)] = np.nan
    return J, g


def polish_adjoint(batch, idx, u, J0, iters, P, cinf):
    """polish_restated.polish with the analytic gradient -> (hist, ties) as there."""
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
        _, g = cost_gradient(f('x0'), f('kparams'), np.asarray(batch['flags'])[idx], u, P)
        g = np.where(np.isfinite(g), g, 0.0)
        ma, md = np.abs(g[:, 0]).max(axis=-1), np.abs(g[:, 1]).max(axis=-1)
        scale = (np.maximum(ma / (4 * ra), md / (4 * rd)) if rd > 0 else ma / (4 * ra)) + 1e-30
        d = -g / scale[:, None, None]
        if not rd > 0:
            d[:, 1] = 0.0
        Uc = R.project(u[:, None] + al[None, :, None, None] * d[:, None], u_prev[:, None, :], P)
        Jc, fc, _ = R.evaluate(batch, idx, Uc, P, cinf)
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
