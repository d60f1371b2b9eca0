"""The Newton (LQ) mode of the polish (igtmpc.h igt_set_polish_step IGT_POLISH_STEP_NEWTON; csrc/igt_kernels_f64.hip
polish_f64_kernel NEWTON, csrc/igt_adjoint64.h Riccati / newton_forward_step) restated in numpy on adjoint_restated's
step_jacobian / cost_gradient and polish_restated's project / evaluate -- tests only.

Per solved scenario and iteration, from the plan u [2, N] with node states X and cost J0:
  1. T_k = step_jacobian(x_k, a_k, df_k) (3 x 5) for every step; g = cost_gradient (non-finite entries 0): the adjoint mode's.
  2. LQ model over z = (ey, epsi, v):  A_k = T_k rows 1-2, columns 0-2, over (0, 0, 1);  B_k = T_k rows 1-2, columns 3-4, over
     (dt, 0);  Q = diag(2, 2, 0), R = 2 w_u I;  the s row enters the linear terms only (the costate of s is -1 throughout):
     q_k = (2 ey_k, 2 epsi_k, 0) - T_k[0, 0:3],  r_k = 2 w_u u_k - T_k[0, 3:5].  The cost is a sum of squares plus a linear
     term, so the model is exact in the cost; only the curvature of the dynamics is dropped (Gauss-Newton).
  3. Riccati sweep from P_N = Q, p_N = (2 ey_N, 2 epsi_N, 0), k = N - 1 .. 0:
        Quu = R + B'PB,  Qux = B'PA,  Qu = r + B'p,  K = -Quu^-1 Qux,  kappa = -Quu^-1 Qu   (2 x 2 inverse by the determinant),
        P <- Q + A'PA + Qux'K, symmetrised (the upper triangle mirrored),  p <- q + A'p + Qux'kappa.
  4. Forward sweep: dz_0 = 0, dN_k = kappa_k + K_k dz_k, dz_k+1 = A_k dz_k + B_k dN_k.  steer_rate = 0: the steering entry of
     dN_k is 0 (before it is propagated).  Non-finite entries of dN become 0; a determinant that is non-finite or <= 0 makes
     the whole dN of that scenario and iteration 0.  dN is not rescaled: trial 0 is the full Newton step.
  5. Trials: lane m < 32 project(u + 2^(-m/3) dN); lane m >= 32 project(u + 2^(-(m-32)/3) dG), dG the adjoint mode's scaled -g.
     Verdicts, the feasible trial of least cost with ties to the lowest m, acceptance only when strictly cheaper: unchanged."""
import numpy as np

import adjoint_restated as A
import np_oracle as O
import polish_restated as R

HALF = R.TRIALS // 2


def lq_model(x0, kp, flags, U, P):
    """x0[n,7] kp[n,3] flags[n] U[n,2,N] -> dict of the LQ model at the plan: A [n,N,3,3], B [n,N,3,2], q [n,N,3], r [n,N,2],
    pN [n,3] (the terminal linear term), Q [3,3], R [2,2]."""
    x0 = O.apply_flags(np.asarray(x0, dtype=np.float64), flags)
    U = np.asarray(U, dtype=np.float64)
    kp = np.asarray(kp, dtype=np.float64)
    n, _, N = U.shape
    X = O.rollout_frenet(x0, U, kp, P)
    xk = np.moveaxis(X[..., :N], -1, -2)                                 # [n, N, 7]
    T = A.step_jacobian(xk, U[:, 0], U[:, 1], kp[:, None, :], P)         # [n, N, 3, 5]
    Am = np.zeros((n, N, 3, 3))
    Am[..., :2, :] = T[..., 1:3, 0:3]
    Am[..., 2, 2] = 1.0
    Bm = np.zeros((n, N, 3, 2))
    Bm[..., :2, :] = T[..., 1:3, 3:5]
    Bm[..., 2, 0] = P.dt
    e = np.stack([2 * X[:, O.IEY], 2 * X[:, O.IEPSI], np.zeros_like(X[:, O.IEY])], axis=-1)     # [n, N + 1, 3]
    q = e[:, :N] - T[..., 0, 0:3]
    r = 2 * P.w_u * np.moveaxis(U, 1, 2) - T[..., 0, 3:5]
    return dict(A=Am, B=Bm, q=q, r=r, pN=e[:, N], Q=np.diag([2.0, 2.0, 0.0]), R=2 * P.w_u * np.eye(2))


def riccati_direction(M, steer=True):
    """the LQ model of lq_model -> dN [n, 2, N], steps 3 and 4 above"""
    Am, Bm, q, r = M['A'], M['B'], M['q'], M['r']
    n, N = q.shape[:2]
    Pm = np.broadcast_to(M['Q'], (n, 3, 3)).copy()
    p = M['pN'].copy()
    K = np.empty((n, N, 2, 3))
    kap = np.empty((n, N, 2))
    ok = np.ones(n, dtype=bool)
    T_ = lambda a: np.swapaxes(a, -1, -2)
    with np.errstate(all='ignore'):
        for k in range(N - 1, -1, -1):
            a, b = Am[:, k], Bm[:, k]
            PB = Pm @ b
            Quu = M['R'] + T_(b) @ PB
            Qux = T_(PB) @ a                                             # B'PA (P symmetric)
            Qu = r[:, k] + np.einsum('nij,ni->nj', b, p)
            det = Quu[:, 0, 0] * Quu[:, 1, 1] - Quu[:, 0, 1] * Quu[:, 1, 0]
            ok &= np.isfinite(det) & (det > 0)
            inv = np.stack([np.stack([Quu[:, 1, 1], -Quu[:, 0, 1]], -1), np.stack([-Quu[:, 1, 0], Quu[:, 0, 0]], -1)], -2) \
                / det[:, None, None]
            K[:, k] = -inv @ Qux
            kap[:, k] = -np.einsum('nij,nj->ni', inv, Qu)
            Pn = M['Q'] + T_(a) @ Pm @ a + T_(Qux) @ K[:, k]
            p = q[:, k] + np.einsum('nij,ni->nj', a, p) + np.einsum('nij,ni->nj', Qux, kap[:, k])
            Pm = np.triu(Pn) + T_(np.triu(Pn, 1))                        # symmetrised: the upper triangle, mirrored
        dz = np.zeros((n, 3))
        d = np.empty((n, 2, N))
        for k in range(N):
            dk = kap[:, k] + np.einsum('nij,nj->ni', K[:, k], dz)
            if not steer:
                dk[:, 1] = 0.0
            d[:, :, k] = dk
            dz = np.einsum('nij,nj->ni', Am[:, k], dz) + np.einsum('nij,nj->ni', Bm[:, k], dk)
    d = np.where(np.isfinite(d), d, 0.0)
    d[~ok] = 0.0
    return d


def dense_direction(M):
    """the minimiser of the same LQ model by the dense normal equations, independent of the recursion: S = d z / d u by
    propagating (A_k, B_k), H = R (x) I + sum S'QS, g_LQ = the model's linear term -> (d [n, 2, N], g_LQ [n, 2, N])"""
    Am, Bm, q, r = M['A'], M['B'], M['q'], M['r']
    n, N = q.shape[:2]
    S = np.zeros((n, 3, N, 2))                                           # d z_k / d u_j, k running
    H = np.zeros((n, N, 2, N, 2))
    g = r.copy()                                                         # [n, N, 2]
    for j in range(N):
        H[:, j, :, j, :] += M['R']
    for k in range(N + 1):
        lin = q[:, k] if k < N else M['pN']
        g += np.einsum('nzju,nz->nju', S, lin)
        H += np.einsum('nzju,zy,nykv->njukv', S, M['Q'], S)
        if k < N:
            S = np.einsum('nzy,nyju->nzju', Am[:, k], S)
            S[:, :, k, :] += Bm[:, k]
    d = np.linalg.solve(H.reshape(n, 2 * N, 2 * N), -g.reshape(n, 2 * N, 1)).reshape(n, N, 2)
    return np.moveaxis(d, 1, 2), np.moveaxis(g, 1, 2)


def newton_direction(x0, kp, flags, U, P):
    return riccati_direction(lq_model(x0, kp, flags, U, P), steer=P.dt * P.steer_rate > 0)


def polish_newton(batch, idx, u, J0, iters, P, cinf):
    """polish_restated.polish with the trial set of step 5 -> (hist, ties) as there."""
    idx = np.asarray(idx)
    u = np.array(u, dtype=np.float64, copy=True)
    J0 = np.array(J0, dtype=np.float64, copy=True)
    n, _, N = u.shape
    ra, rd = P.dt * P.jerk, P.dt * P.steer_rate
    f = lambda k: np.asarray(batch[k], dtype=np.float64)[idx]
    u_prev = f('u_prev')
    flags = np.asarray(batch['flags'])[idx]
    alive = np.ones(n, dtype=bool)
    hist, ties = [(u.copy(), J0.copy())], []
    al = 2.0 ** (-np.arange(HALF) / 3.0)
    for _ in range(iters):
        _, g = A.cost_gradient(f('x0'), f('kparams'), flags, u, P)
        g = np.where(np.isfinite(g), g, 0.0)
        ma, md = np.abs(g[:, 0]).max(axis=-1), np.abs(g[:, 1]).max(axis=-1)
        scale = (np.maximum(ma / (4 * ra), md / (4 * rd)) if rd > 0 else ma / (4 * ra)) + 1e-30
        dG = -g / scale[:, None, None]
        if not rd > 0:
            dG[:, 1] = 0.0
        dN = newton_direction(f('x0'), f('kparams'), flags, u, P)
        steps = np.concatenate([al[None, :, None, None] * dN[:, None], al[None, :, None, None] * dG[:, None]], axis=1)
        Uc = R.project(u[:, None] + steps, u_prev[:, None, :], P)
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
