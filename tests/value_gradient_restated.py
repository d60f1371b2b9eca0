"""The terminal value of the gt_mpc cost with its partials (igtmpc.h igt_terminal_value_f64) and the analytic gradient of the
value-network cost (igt_cost_gradient_vn_f64) restated in numpy on the oracle's model -- tests only.

V_out(s_N, v_N) = V(Wn (x_N - mu_f)) sigma_t + mu_t with x_N = np_oracle.value_features: only features 3 (s_N - s_tv) and 4
(v_N - v_tv) depend on the plan, so the whitened input moves along columns 3 and 4 of Wn, and through every hidden layer
y = W h + b, h = tanh(y) the chain rule is h' = (1 - h^2) (W h'_prev); the output layer is linear and sigma_t scales the result.

J(u) = sum_{k<=N} (epsi_k^2 + ey_k^2) + w_u sum_{k<N} (a_k^2 + df_k^2) - V_out(s_N, v_N): the costate recursion of
adjoint_restated.cost_gradient from the terminal seed (-dV_out/ds_N, 2 ey_N, 2 epsi_N, -dV_out/dv_N) -- v_N = v_0 + dt sum a_k, so
the v entry reaches every a_k through the dt lam_v term of the step."""
import numpy as np

import adjoint_restated as A
import np_oracle as O


def terminal_value_and_partials(net, sv, tv_sv, enc):
    """net = dict(layers, Wn[6,6], mu_f[6], sigma_t, mu_t); sv[n,2] = (s_N, v_N), tv_sv[n,2], enc[n,2]
    -> (V_out[n], dV_out[n,2] = d V_out / d (s_N, v_N))."""
    sv, tv_sv, enc = (np.asarray(q, dtype=np.float64) for q in (sv, tv_sv, enc))
    layers = [(np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)) for W, b in net['layers']]
    Wn = np.asarray(net['Wn'], dtype=np.float64)
    with np.errstate(all='ignore'):
        f = O.value_features(sv[:, 0:1], sv[:, 1:2], tv_sv, enc)[:, 0]             # [n, 6]
        z = (f - np.asarray(net['mu_f'], dtype=np.float64)) @ Wn.T
        V = O.value_net_forward(layers, z)[..., 0] * net['sigma_t'] + net['mu_t']
        t = np.broadcast_to(Wn[:, 3:5], (len(z), 6, 2))                             # d z / d (s_N, v_N)
        for li, (W, _) in enumerate(layers):
            t = np.einsum('oi,nic->noc', W, t)
            if li + 1 < len(layers):
                h = np.tanh(O.value_net_forward(layers[:li + 1], z))                # a prefix ends without tanh: the layer's y
                t = (1.0 - h * h)[..., None] * t
        dV = t[:, 0, :] * net['sigma_t']
    return V, dV


def cost_vn(x0, kp, flags, tv_sv, enc, U, P, net):
    """J[B] alone: np_oracle.stage_cost with the terminal value of the roll-out's own (s_N, v_N)."""
    x0 = O.apply_flags(np.asarray(x0, dtype=np.float64), flags)
    N = U.shape[-1]
    with np.errstate(all='ignore'):
        X = O.rollout_frenet(x0, U, kp, P)
        V = O.terminal_value(net, X[:, None, O.IS, N], X[:, None, O.IV, N], tv_sv, enc)[:, 0]
        return O.stage_cost(X, U, P, terminal_value=V)


def cost_gradient_vn(x0, kp, flags, tv_sv, enc, U, P, net):
    """x0[B,7] kp[B,3] flags[B] tv_sv[B,2] enc[B,2] U[B,2,N] -> (J[B], g[B,2,N]); no projection, no verdicts; a non-finite cost
    gives a NaN row."""
    x0 = O.apply_flags(np.asarray(x0, dtype=np.float64), flags)
    U = np.asarray(U, dtype=np.float64)
    kp = np.asarray(kp, dtype=np.float64)
    N = U.shape[-1]
    with np.errstate(all='ignore'):
        X = O.rollout_frenet(x0, U, kp, P)
        V, dV = terminal_value_and_partials(net, np.stack([X[:, O.IS, N], X[:, O.IV, N]], axis=-1), tv_sv, enc)
        J = O.stage_cost(X, U, P, terminal_value=V)
        g = np.empty_like(U)
        lam = np.stack([-dV[:, 0], 2 * X[..., O.IEY, N], 2 * X[..., O.IEPSI, N], -dV[:, 1]], axis=-1)
        for k in range(N - 1, -1, -1):
            T = A.step_jacobian(X[..., :, k], U[..., 0, k], U[..., 1, k], kp, P)
            c = np.einsum('...rd,...r->...d', T, lam[..., :3])
            g[..., 0, k] = 2 * P.w_u * U[..., 0, k] + c[..., 3] + P.dt * lam[..., 3]
            g[..., 1, k] = 2 * P.w_u * U[..., 1, k] + c[..., 4]
            lam = np.stack([lam[..., 0], 2 * X[..., O.IEY, k] + c[..., 0], 2 * X[..., O.IEPSI, k] + c[..., 1],
                            lam[..., 3] + c[..., 2]], axis=-1)
    g[~np.isfinite(J)] = np.nan
    return J, g
