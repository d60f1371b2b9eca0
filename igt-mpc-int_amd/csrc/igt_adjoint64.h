// igt_adjoint64.h -- the derivative of one control step of the RK4 Frenet model, float64 (gfx950): what the cost gradient
// (igt_kernels_f64.hip cost_gradient_f64_kernel, igt_cost_gradient_f64) and the adjoint mode of the polish (polish_f64_kernel,
// igt_set_polish_gradient) are made of; at the end of the file the Riccati and forward steps of the polish's Newton direction
// (igt_set_polish_step) over the same Jacobians.
//
// The progress cost (mpc.py:356-373) reads (s, ey, epsi) and the inputs only, so the Cartesian rows are left out; s feeds back
// through the piecewise-constant K(s) alone, which is taken as locally constant -- the derivative wherever no RK stage argument
// sits on a break-point -- so d x_k+1 / d s_k is the unit column; and v_k+1 = v_k + dt a_k.  What remains of one control step's
// Jacobian is five tangent directions (ey, epsi, v, a, df) over the three rows (s, ey, epsi):
//     T[r][0..2] = A_k  (d row r of x_k+1 / d (ey, epsi, v) of x_k),     T[r][3..4] = B_k  (d row r of x_k+1 / d (a_k, df_k)).
// Arithmetic: forward mode through the reference's own stage functions (kinematic_bicycle_model_frenet.py:70-127, the
// operations of ExactStepper<double>, igt_device.h), NOT through the factorised Fast64 sub-step: the tangents of Fast64's
// carried rotations and stage-sum factorisation would be a second derivation to keep in step with the first, while here every
// line is the textbook partial of the line above it.  The price is one sincos of epsi per RK stage (16 per control step at
// n_rk4 = 4) instead of one per control step; the slip angle's pair comes from slip() once per step and each stage's
// (sin, cos)(beta + epsi') by the angle sum.  Values and tangents are accurate to double rounding (no truncated series), for any
// n_rk4; nothing here is bit-equal to the roll-out of igt_fast64.h, and nothing needs to be: the gradient is compared at 1e-9,
// the roll-outs agree with this forward sweep to ~1e-13.  Every fused multiply-add is written out (-ffp-contract=off).
// No wave votes, no LDS: a lane calls it for a step of its own.
#pragma once
#include "igt_device.h"
#include "igt_math64.h"

namespace igt {
namespace adj {

using m64::rcp_nr;
using m64::rsq_nr;
using m64::sincos_reduced;

// (sin, cos) of the slip angle beta = atan(r tan df) as igt_fast64.h slip_trig forms them, and d beta / d df = r / (cos^2 df + r^2 sin^2 df)
struct Slip {
    double sb, cb, dbeta;
};
__device__ __forceinline__ Slip slip(double lr_ratio, double df) {
    double sdf, cdf;
    sincos_reduced(df, sdf, cdf);
    const double n = rsq_nr(fma((lr_ratio * lr_ratio) * sdf, sdf, cdf * cdf));      // argument in [r^2, 1]
    Slip sl;
    sl.cb = cdf * n;
    sl.sb = lr_ratio * sdf * n;
    sl.dbeta = lr_ratio * (n * n);
    return sl;
}

struct StepModel {
    double h, hh, h6, dt, inv_lr, lr_ratio, b0, b1, kv;
    int n_rk4;

    __device__ __forceinline__ void init(const KP& P, double b0_, double b1_, double kv_) {
        h = P.h; hh = P.h / 2; h6 = P.h / 6; dt = P.dt;
        inv_lr = 1.0 / P.l_r; lr_ratio = P.lr_ratio;
        b0 = b0_; b1 = b1_; kv = kv_; n_rk4 = P.n_rk4;
    }

    // one RK stage at (s, ey, ep, v): the derivative rows (frenet.py:73-79) and their partials
    struct Stage {
        double ks, ke, kp;                    // ds/dt, dey/dt, depsi/dt
        double s_ey, s_th, s_v, e_th, e_v;    // partials of ks by ey, by the angle beta + epsi, by v; of ke by the angle, by v
        double K;
    };
    __device__ __forceinline__ void stage(double s, double ey, double ep, double v, const Slip& sl, Stage& g) const {
        const double K = ((s >= b0) ? kv : 0.0) - ((s >= b1) ? kv : 0.0);           // mpc.py:199 pw_const
        double se, ce;
        sincos_reduced(ep, se, ce);
        const double sn = fma(se, sl.cb, ce * sl.sb);                                 // sin(beta + epsi)
        const double cs = fma(ce, sl.cb, -(se * sl.sb));                              // cos(beta + epsi)
        const double D = rcp_nr(fma(-K, ey, 1.0));
        const double cD = cs * D;
        g.K = K;
        g.ks = v * cD;                                                                // :73
        g.ke = v * sn;                                                                // :76
        g.kp = fma(-K, g.ks, v * (sl.sb * inv_lr));                                   // :79
        g.s_ey = (g.ks * D) * K;
        g.s_th = -(g.ke * D);
        g.s_v = cD;
        g.e_th = v * cs;
        g.e_v = sn;
    }

    // One control step from (s, ey, ep, v) with (a, slip of df): the state rows advance in place (v is the caller's: v + dt a).
    // JAC: T[3][5] returns the step's Jacobian, rows (s, ey, epsi), columns (ey, epsi, v, a, df) -- step_jacobian below.
    template <bool JAC>
    __device__ __forceinline__ void step(double& s, double& ey, double& ep, double v, double a, const Slip& sl,
                                         double (&T)[3][5]) const {
        if (JAC) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int d = 0; d < 5; ++d) T[r][d] = (r == 1 && d == 0) || (r == 2 && d == 1) ? 1.0 : 0.0;
        }
        const double sblr = sl.sb * inv_lr;
        const double cblr = sl.cb * inv_lr * sl.dbeta;           // d (sin(beta) / l_r) / d df
        for (int j = 0; j < n_rk4; ++j) {                        // :107
            const double tau = (double)j * h;                    // d v / d a at the sub-step's start
            double ps = 0.0, pe = 0.0, pp = 0.0;                 // the stage before: values ...
            double pt[3][5];                                     // ... and tangents
            double as = 0.0, ae = 0.0, ap = 0.0;                 // weighted sums (1, 2, 2, 1)
            double at[3][5];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const double c = st == 3 ? h : hh;               // offset of this stage's arguments (none at st = 0)
                const double wg = (st == 1 || st == 2) ? 2.0 : 1.0;
                const double vs = st == 0 ? v : fma(c, a, v);
                Stage g;
                if (st == 0) stage(s, ey, ep, vs, sl, g);
                else stage(fma(c, ps, s), fma(c, pe, ey), fma(c, pp, ep), vs, sl, g);
                if (JAC) {
                    const double tv = st == 0 ? tau : tau + c;   // direction a: d v' / d a
#pragma unroll
                    for (int d = 0; d < 5; ++d) {
                        const double tey = st == 0 ? T[1][d] : fma(c, pt[1][d], T[1][d]);
                        double th = st == 0 ? T[2][d] : fma(c, pt[2][d], T[2][d]);
                        if (d == 4) th += sl.dbeta;              // the angle is beta + epsi
                        double ns = fma(g.s_ey, tey, g.s_th * th);
                        double ne = g.e_th * th;
                        double np = 0.0;
                        if (d == 2) { ns += g.s_v; ne += g.e_v; np = sblr; }
                        if (d == 3) { ns = fma(g.s_v, tv, ns); ne = fma(g.e_v, tv, ne); np = sblr * tv; }
                        if (d == 4) np = vs * cblr;
                        np = fma(-g.K, ns, np);
                        pt[0][d] = ns; pt[1][d] = ne; pt[2][d] = np;
                        if (st == 0) { at[0][d] = ns; at[1][d] = ne; at[2][d] = np; }
                        else { at[0][d] = fma(wg, ns, at[0][d]); at[1][d] = fma(wg, ne, at[1][d]); at[2][d] = fma(wg, np, at[2][d]); }
                    }
                }
                ps = g.ks; pe = g.ke; pp = g.kp;
                as = fma(wg, ps, as); ae = fma(wg, pe, ae); ap = fma(wg, pp, ap);
            }
            s = fma(h6, as, s); ey = fma(h6, ae, ey); ep = fma(h6, ap, ep);         // :113-115
            v = fma(h, a, v);                                                        // :116
            if (JAC) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int d = 0; d < 5; ++d) T[r][d] = fma(h6, at[r][d], T[r][d]);
            }
        }
    }
};

// A_k, B_k of one control step at x_k = (s, ey, ep, v) with (a_k, df_k), any n_rk4: T[r][0..2] = A_k, T[r][3..4] = B_k (see the
// head of this file; the s column of A_k is the unit column and the v row is (0, 0, 0, 1 | dt, 0): neither is stored)
__device__ __forceinline__ void step_jacobian(const StepModel& M, double s, double ey, double ep, double v, double a, double df,
                                              double (&T)[3][5]) {
    const Slip sl = slip(M.lr_ratio, df);
    M.template step<true>(s, ey, ep, v, a, sl, T);
}

// The costate of the progress cost one step back: lam = (d J / d s, ey, epsi, v) at node k + 1 becomes that at node k, and
// (ga, gd) = d J / d (a_k, df_k).  J's own terms at node k: ey_k^2 + epsi_k^2 + w_u (a_k^2 + df_k^2)   (mpc.py:361-364).
__device__ __forceinline__ void costate_step(const double (&T)[3][5], double dt, double w_u, double ey, double ep, double a, double df,
                                             double (&lam)[4], double& ga, double& gd) {
    double c[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) c[d] = fma(T[2][d], lam[2], fma(T[1][d], lam[1], T[0][d] * lam[0]));
    ga = fma(2.0 * w_u, a, fma(dt, lam[3], c[3]));
    gd = fma(2.0 * w_u, df, c[4]);
    lam[1] = fma(2.0, ey, c[0]);
    lam[2] = fma(2.0, ep, c[1]);
    lam[3] = lam[3] + c[2];
}

// ---- the Newton (LQ) direction of the polish (igt_set_polish_step IGT_POLISH_STEP_NEWTON) ----
// The Gauss-Newton model of the progress cost around the plan, over z = (ey, epsi, v): A_k = rows (ey, epsi) of T_k, columns
// 0..2, over (0, 0, 1); B_k = the same rows, columns 3..4, over (dt, 0); Q = diag(2, 2, 0), R = 2 w_u I.  The s row of T_k
// enters the linear terms only (the costate of s is -1 throughout): q_k = (2 ey_k, 2 epsi_k, 0) - T_k[0][0..2],
// r_k = 2 w_u u_k - T_k[0][3..4].  The cost is a sum of squares plus a linear term, so the model is exact in the cost; only
// the curvature of the dynamics is dropped.  The unit row of A_k and the (dt, 0) row of B_k are written as what they are.
struct Riccati {
    double P[3][3], p[3];      // the quadratic and linear terms of the cost-to-go at node k + 1, then at node k
    bool ok;                   // every determinant so far was finite and > 0

    __device__ __forceinline__ void init(double eyN, double epN) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) P[i][j] = (i == j && i < 2) ? 2.0 : 0.0;
        p[0] = 2.0 * eyN; p[1] = 2.0 * epN; p[2] = 0.0;
        ok = true;
    }

    // one step back: Quu = R + B'PB, Qux = B'PA, Qu = r + B'p, K = -Quu^-1 Qux, kap = -Quu^-1 Qu (the 2 x 2 inverse by the
    // determinant), P <- Q + A'PA + Qux'K, p <- q + A'p + Qux'kap.  P is symmetric and kept so: Quu's and the new P's upper
    // triangles are formed and mirrored (the symmetrisation), which is also a third of the multiply-adds less.
    __device__ __forceinline__ void step(const double (&T)[3][5], double dt, double w_u, double ey, double ep, double a, double df,
                                         double (&K)[2][3], double (&kap)[2]) {
        double W[3][3], PB[3][2];                                // P A, P B
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                W[i][j] = fma(P[i][1], T[2][j], P[i][0] * T[1][j]);
                if (j == 2) W[i][j] += P[i][2];
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                PB[i][c] = fma(P[i][1], T[2][3 + c], P[i][0] * T[1][3 + c]);
                if (c == 0) PB[i][c] = fma(P[i][2], dt, PB[i][c]);
            }
        }
        double Quu[2][2], Qux[2][3], Qu[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int d = c; d < 2; ++d) {
                Quu[c][d] = fma(T[2][3 + c], PB[1][d], T[1][3 + c] * PB[0][d]);
                if (c == 0) Quu[c][d] = fma(dt, PB[2][d], Quu[c][d]);
                if (c == d) Quu[c][d] += 2.0 * w_u;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                Qux[c][j] = fma(T[2][3 + c], W[1][j], T[1][3 + c] * W[0][j]);
                if (c == 0) Qux[c][j] = fma(dt, W[2][j], Qux[c][j]);
            }
            Qu[c] = fma(T[2][3 + c], p[1], T[1][3 + c] * p[0]);
            if (c == 0) Qu[c] = fma(dt, p[2], Qu[c]);
            Qu[c] += fma(2.0 * w_u, c == 0 ? a : df, -T[0][3 + c]);
        }
        const double det = fma(Quu[0][0], Quu[1][1], -(Quu[0][1] * Quu[0][1]));
        ok = ok && fabs(det) < 1.79e308 && det > 0.0;
        const double nid = -rcp_nr(det);                         // -Quu^-1 = nid (Quu11, -Quu01; -Quu01, Quu00)
        const double I00 = Quu[1][1] * nid, I01 = -(Quu[0][1] * nid), I11 = Quu[0][0] * nid;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            K[0][j] = fma(I01, Qux[1][j], I00 * Qux[0][j]);
            K[1][j] = fma(I11, Qux[1][j], I01 * Qux[0][j]);
        }
        kap[0] = fma(I01, Qu[1], I00 * Qu[0]);
        kap[1] = fma(I11, Qu[1], I01 * Qu[0]);
        double pn[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double v = fma(T[2][i], p[1], T[1][i] * p[0]);                           // A'p
            if (i == 2) v += p[2];
            v = fma(Qux[1][i], kap[1], fma(Qux[0][i], kap[0], v));
            pn[i] = v + (i == 0 ? fma(2.0, ey, -T[0][0]) : i == 1 ? fma(2.0, ep, -T[0][1]) : -T[0][2]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i; j < 3; ++j) {
                double v = fma(T[2][i], W[1][j], T[1][i] * W[0][j]);                 // A'PA
                if (i == 2) v += W[2][j];
                v = fma(Qux[1][i], K[1][j], fma(Qux[0][i], K[0][j], v));
                if (i == j && i < 2) v += 2.0;
                P[i][j] = v;                                                         // W, PB hold what is needed of the old P
                P[j][i] = v;
            }
            p[i] = pn[i];
        }
    }
};

// The forward sweep's step: d = kap_k + K_k dz (steer false: the steering entry is 0), dz <- A_k dz + B_k d.  T: rows 1, 2 are read.
__device__ __forceinline__ void newton_forward_step(const double (&T)[3][5], double dt, const double (&K)[2][3], const double (&kap)[2],
                                                    bool steer, double (&dz)[3], double (&d)[2]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) d[c] = fma(K[c][2], dz[2], fma(K[c][1], dz[1], fma(K[c][0], dz[0], kap[c])));
    if (!steer) d[1] = 0.0;
    double nz[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
        nz[i] = fma(T[1 + i][4], d[1], fma(T[1 + i][3], d[0], fma(T[1 + i][2], dz[2], fma(T[1 + i][1], dz[1], T[1 + i][0] * dz[0]))));
    dz[0] = nz[0]; dz[1] = nz[1];
    dz[2] = fma(dt, d[0], dz[2]);
}

}  // namespace adj
}  // namespace igt
