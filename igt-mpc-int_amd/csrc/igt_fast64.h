// igt_fast64.h -- the float64 rollout of the search / emit / rollout-all kernels of the _f64 entry points (gfx950).
//
// The reference is float64 end to end (kinematic_bicycle_model_frenet.py:70-127, mpc.py:356-373), so this is the path
// that runs at the reference's precision.  It evaluates the same RK4 stages as ExactStepper<double> (igt_device.h,
// the oracle's operation order) but with the algebra of the float path (igt_fast_impl.inc) carried out in double:
//   * v and psi do not feed back: stage speeds and the psi offsets are closed-form;
//   * sin/cos of (beta+epsi') and (psi'+beta) are rotations of the sub-step's base pair by the stage offset, the
//     offset's sine / cosine from a Taylor polynomial (|offset| <= h |rate| << 1; truncation < 1e-17 relative);
//     libm-grade sincos is evaluated once per control step (of the slip angle) instead of 32 times -- the (beta + epsi)
//     and (psi + beta) pairs are carried from step to step by rotations and renormalised;
//   * all weighted stage sums are factorised, sum_j w_j g_j cos(theta + d_j) = cos(theta) A - sin(theta) B, for the
//     Frenet rows and the Cartesian rows (the latter including the reference's quirk that stage 4 sees
//     psi + h/2 k3[6], kinematic_bicycle_model_frenet.py:111);
//   * beta = atan(r tan df) is never formed: cos(beta) = c/n, sin(beta) = r s/n, n = sqrt(c^2 + r^2 s^2);
//   * K(s') is decided on (s - b) + offset >= 0 (the oracle compares s + offset >= b).
// Nothing is approximated beyond double rounding: measured <= 1e-12 against the reference-generated golden
// rollouts (curvature break-point straddlers included), i.e. three orders inside the 1e-9 bar of the _f64 tests.
// Three variants of a sub-step (K == 0 everywhere / K == kv everywhere / general), chosen by wave votes on a travel
// bound, are bit-identical wherever they apply (x - 0, x * 1, rotation by (0, 1) are exact), so search (votes),
// emit (general variant, lanes of different scenarios) and rollout-all agree bit for bit -- asserted in the tests.
#pragma once
#include "igt_device.h"
#include "igt_math64.h"
#include "igt_roll_options.h"

namespace igt {
namespace f64 {

using m64::sincos_kernel;
using m64::sincos_reduced;
using m64::QUADRANT0;
using m64::rcp_nr;
using m64::rsq_nr;


// ---- sin/cos of a small stage offset ---------------------------------------------------------------------------
// |d| <= 0.15: sin to d^9, cos to d^10 (first dropped terms 2e-17 / 2e-19 relative to 1)
__device__ __forceinline__ void small_sincos(double d, double& sd, double& cd) {
    const double d2 = d * d;
    double p = fma(d2, 1.0 / 362880.0, -1.0 / 5040.0);
    p = fma(d2, p, 1.0 / 120.0);
    p = fma(d2, p, -1.0 / 6.0);
    sd = fma(d * d2, p, d);
    double q = fma(d2, -1.0 / 3628800.0, 1.0 / 40320.0);
    q = fma(d2, q, -1.0 / 720.0);
    q = fma(d2, q, 1.0 / 24.0);
    q = fma(d2, q, -0.5);
    cd = fma(d2, q, 1.0);
}
// |d| <= 0.6 (coarse discretisations, n_rk4 <= 2): two more terms each
__device__ __forceinline__ void small_sincos_hi(double d, double& sd, double& cd) {
    const double d2 = d * d;
    double p = fma(d2, 1.0 / 6227020800.0, -1.0 / 39916800.0);
    p = fma(d2, p, 1.0 / 362880.0);
    p = fma(d2, p, -1.0 / 5040.0);
    p = fma(d2, p, 1.0 / 120.0);
    p = fma(d2, p, -1.0 / 6.0);
    sd = fma(d * d2, p, d);
    double q = fma(d2, -1.0 / 87178291200.0, 1.0 / 479001600.0);
    q = fma(d2, q, -1.0 / 3628800.0);
    q = fma(d2, q, 1.0 / 40320.0);
    q = fma(d2, q, -1.0 / 720.0);
    q = fma(d2, q, 1.0 / 24.0);
    q = fma(d2, q, -0.5);
    cd = fma(d2, q, 1.0);
}

__device__ __forceinline__ void rotate(double& s, double& c, double sd, double cd) {
    const double s_ = fma(s, cd, c * sd);
    const double c_ = fma(c, cd, -(s * sd));
    s = s_; c = c_;
}
// NRK: the number of RK4 sub-steps per control step as a compile-time constant (4: what evaluate.py:109,440 passes), or 0:
// read from the parameters at run time.  With it fixed the generic sub-step loops vanish from the kernel and so does the
// register pressure they add: the control step of a straight route is 410 instructions instead of 464 (ISA count).
template <bool HI_ORDER, int NRK = 0>
struct Fast64 {
    double h, hh, h6, kv, inv_lr, lr_ratio, b0, b1, dt;
    int n_rk4;
    __device__ __forceinline__ int nrk() const { return NRK > 0 ? NRK : n_rk4; }

    __device__ __forceinline__ void init(const KP& P, double b0_, double b1_, double kv_) {
        h = P.h; hh = P.h / 2; h6 = P.h / 6;
        kv = kv_; inv_lr = 1.0 / P.l_r; lr_ratio = P.lr_ratio;
        b0 = b0_; b1 = b1_; dt = P.dt; n_rk4 = P.n_rk4;
    }
    static __device__ __forceinline__ void ssc(double d, double& sd, double& cd) {
        if (HI_ORDER) small_sincos_hi(d, sd, cd); else small_sincos(d, sd, cd);
    }
    // curvature at the break-point-relative argument d + o  (mpc.py:199 pw_const: kv [s >= b0] - kv [s >= b1])
    __device__ __forceinline__ double curv(double d0, double d1, double o) const {
        return ((d0 + o >= 0.0) ? kv : 0.0) - ((d1 + o >= 0.0) ? kv : 0.0);
    }

    // working set of one control step: base pairs (s1,c1) = (sin,cos)(beta+epsi), (s2,c2) = (sin,cos)(psi+beta);
    // v1, ey and the break-point-relative arc lengths d0, d1 advance per sub-step; acc_* are the step's increments
    struct Work {
        double s1, c1, s2, c2, v1, ey, d0, d1, acc_s, acc_ey, acc_ep, acc_x, acc_y, acc_psi;
        double sh, ch;        // (sin,cos)(h/2 w2) of the current sub-step, carried by rotation (see StepConst)
    };
    // The psi offsets of a control step form an arithmetic progression: w = v sin(beta)/l_r is linear in v and v advances
    // by h/2 a per half sub-step, so with delta = h/2 * (h/2 a) * sin(beta)/l_r
    //     h/2 w1 = h/2 w2 - delta,   h w2 = 2 (h/2 w2),   next sub-step: h/2 w2' = h/2 w2 + 2 delta.
    // One polynomial per CONTROL step (h/2 w2 of the first sub-step) plus rotations by +-delta / 2 delta and a double-angle
    // replace three polynomials per SUB-step -- the same numbers in every sub-step variant (mode-independent code).
    struct StepConst {
        double ha, sblr, sd, cd, s2d, c2d;
    };

    // A = g1 + 2 g2 cdA + 2 g3 cdB + g4 cdC,  B = 2 g2 sdA + 2 g3 sdB + g4 sdC   (weights 1,2,2,1)
    static __device__ __forceinline__ void stage_sums(double g1, double g2, double g3, double g4, double sdA, double cdA,
                                                      double sdB, double cdB, double sdC, double cdC, double& A, double& B) {
        const double t2 = 2.0 * g2, t3 = 2.0 * g3;
        A = fma(g4, cdC, fma(t3, cdB, fma(t2, cdA, g1)));
        B = fma(g4, sdC, fma(t3, sdB, t2 * sdA));
    }

    // MODE 0: general (K decided per stage argument); 1: K == 0 at every stage argument of every lane; 2: every stage
    // argument of every lane lies strictly inside the arc, K == kv.  All three give identical bits where they apply.
    // XY = false (search units whose obstacles are out of every candidate's reach): the Cartesian rows are not integrated
    // KEEP_D = false (MODE 1, a whole control step taken as K == 0): d0, d1 are left alone -- nothing reads them before
    // step_head sets them again from s (substeps)
    template <int MODE, bool XY = true, bool KEEP_D = true>
    __device__ __forceinline__ void substep(const StepConst& sc, Work& w) const {
        static_assert(KEEP_D || MODE == 1, "only the K == 0 variant reads neither d0 nor d1");
        constexpr bool K0 = MODE == 1, KC = MODE == 2;
        const double ha = sc.ha, sblr = sc.sblr;
        const double v1 = w.v1;
        const double v2 = v1 + ha;            // stages 2,3
        const double v4 = v2 + ha;            // stage 4
        const double s1 = w.s1, c1 = w.c1;
        const double w1 = v1 * sblr, w2 = v2 * sblr, w4 = v4 * sblr;
        // psi offsets h/2 w1 (stage 2), h/2 w2 (stages 3 AND 4, frenet.py:111), h w2 (the sub-step's psi advance)
        const double sd3 = w.sh, cd3 = w.ch;
        double sd2 = sd3, cd2 = cd3;
        rotate(sd2, cd2, -sc.sd, sc.cd);
        const double sdP = 2.0 * sd3 * cd3, cdP = fma(-2.0 * sd3, sd3, 1.0);
        double As, Bs, Ae, Be, sdC, cdC, corr = 0.0;
        if (K0) {
            // 1 - K ey = 1 and depsi = dpsi: the (beta+epsi) stage offsets are the psi offsets, the gains the speeds
            sdC = sdP; cdC = cdP;
            stage_sums(v1, v2, v2, v4, sd2, cd2, sd3, cd3, sdC, cdC, Ae, Be);
            As = Ae; Bs = Be;
        } else {
            const double ey = w.ey, d0 = w.d0, d1 = w.d1;
            double sdA, cdA, sdB, cdB, sa, ca;
            // ---- stage 1                                                            (frenet.py:73-79)
            double K = KC ? kv : curv(d0, d1, 0.0);
            const double g1 = v1 * rcp_nr(fma(-K, ey, 1.0));
            const double ds1 = g1 * c1;
            const double de1 = v1 * s1;
            const double kd1 = ds1 * K;
            // ---- stage 2: arguments base + h/2 k1; its offset h/2 dp1 = h/2 w1 - h/2 kd1: the psi offset turned back by
            //      the curvature part (kd == 0 turns by (0, 1): exactly the psi offset, as the K == 0 variant uses)
            {
                double sk, ck;
                ssc(-(hh * kd1), sk, ck);
                sdA = sd2; cdA = cd2; rotate(sdA, cdA, sk, ck);
            }
            sa = s1; ca = c1; rotate(sa, ca, sdA, cdA);
            if (!KC) K = curv(d0, d1, hh * ds1);
            const double g2 = v2 * rcp_nr(fma(-K, fma(hh, de1, ey), 1.0));
            const double ds2 = g2 * ca;
            const double de2 = v2 * sa;
            const double kd2 = ds2 * K;
            // ---- stage 3: base + h/2 k2
            {
                double sk, ck;
                ssc(-(hh * kd2), sk, ck);
                sdB = sd3; cdB = cd3; rotate(sdB, cdB, sk, ck);
            }
            sa = s1; ca = c1; rotate(sa, ca, sdB, cdB);
            if (!KC) K = curv(d0, d1, hh * ds2);
            const double g3 = v2 * rcp_nr(fma(-K, fma(hh, de2, ey), 1.0));
            const double ds3 = g3 * ca;
            const double de3 = v2 * sa;
            const double kd3 = ds3 * K;
            // ---- stage 4: base + h k3 (only its cosine is needed individually, for depsi)
            {
                double sk, ck;
                ssc(-(h * kd3), sk, ck);
                sdC = sdP; cdC = cdP; rotate(sdC, cdC, sk, ck);
            }
            if (!KC) K = curv(d0, d1, h * ds3);
            const double g4 = v4 * rcp_nr(fma(-K, fma(h, de3, ey), 1.0));
            const double ds4 = g4 * fma(c1, cdC, -(s1 * sdC));
            const double kd4 = ds4 * K;
            stage_sums(g1, g2, g3, g4, sdA, cdA, sdB, cdB, sdC, cdC, As, Bs);
            stage_sums(v1, v2, v2, v4, sdA, cdA, sdB, cdB, sdC, cdC, Ae, Be);
            corr = h6 * (kd1 + 2.0 * kd2 + 2.0 * kd3 + kd4);        // curvature part of the epsi increment
        }
        const double ip = h * w2 - corr;                             // K == 0: h w2 - 0, the same bits
        // ---- Frenet increments (frenet.py:113-115)
        const double is = h6 * fma(c1, As, -(s1 * Bs));
        const double ie = h6 * fma(s1, Ae, c1 * Be);
        // ---- Cartesian rows collapse to one rotation of (A,B) as well (stage 4 shares stage 3's offset)
        if (XY) {
            const double v34 = fma(2.0, v2, v4);
            const double tv2 = 2.0 * v2;
            const double Ac = fma(v34, cd3, fma(tv2, cd2, v1));
            const double Bc = fma(v34, sd3, tv2 * sd2);
            w.acc_x = fma(h6, fma(w.c2, Ac, -(w.s2 * Bc)), w.acc_x);
            w.acc_y = fma(h6, fma(w.s2, Ac, w.c2 * Bc), w.acc_y);
        }
        w.acc_psi = fma(h6, w1 + 4.0 * w2 + w4, w.acc_psi);
        w.acc_s += is; w.acc_ey += ie; w.acc_ep += ip;
        if (KEEP_D) { w.d0 += is; w.d1 += is; }
        w.ey += ie; w.v1 = v4;
        // ---- base pairs for the next sub-step: (psi+beta) advances by h w2, (beta+epsi) by h w2 - corr: the psi
        // advance turned back by corr.  K == 0: corr = 0 exactly, the extra turn is by (0, 1) -- bit-identical variants.
        if (XY) rotate(w.s2, w.c2, sdP, cdP);
        rotate(w.s1, w.c1, sdP, cdP);
        if (!K0) {
            double sk, ck;
            ssc(-corr, sk, ck);
            rotate(w.s1, w.c1, sk, ck);
        }
        rotate(w.sh, w.ch, sc.s2d, sc.c2d);                          // h/2 w2 of the next sub-step
    }

    // n_rk4 sub-steps of one control step.  The K == 0 variant (or the K == kv one) is taken when it is provably
    // exact for every active lane of the wave: straight route, or every lane's stage arguments stay outside (inside)
    // the arc [b0, b1] by the travel bound |ds| <= 2 |v| (1/(1 - K ey) < 2 while |K ey| < 1/2: part of the "inside" vote --
    // found by the N = 64 fuzz draws of round 4: an infeasible candidate 6 m off the road travelled 3.5 |v| dt in a step).
    // UNIFORM = false (emit: the lanes of a wave belong to different scenarios): the same choice by votes over the lanes.
    // the n_rk4 sub-steps of one variant; the reference's discretisation (4) is unrolled: no loop-carried register copies
    template <int MODE, bool XY, bool KEEP_D = true>
    __device__ __forceinline__ void run(const StepConst& sc, Work& w) const {
        if (NRK == 4 || (NRK == 0 && n_rk4 == 4)) {
            substep<MODE, XY, KEEP_D>(sc, w); substep<MODE, XY, KEEP_D>(sc, w);
            substep<MODE, XY, KEEP_D>(sc, w); substep<MODE, XY, KEEP_D>(sc, w);
        } else {
            for (int j = 0; j < nrk(); ++j) substep<MODE, XY, KEEP_D>(sc, w);
        }
    }

    // the constants of one control step (and the first sub-step's (sin, cos)(h/2 w2) in w): the same statements for the
    // search / emit / rollout-all roll-outs and for the Cartesian rows rolled on their own (cartesian_rows)
    __device__ __forceinline__ StepConst step_const(double a, double sblr, Work& w) const {
        const double ha = hh * a;
        StepConst sc;
        sc.ha = ha; sc.sblr = sblr;
        {   // delta = h/2 (w2 - w1) = (h/2)^2 a sin(beta)/l_r is tiny (< 4e-3 even at h = 0.1): sin to d^5, cos to d^4
            const double d = hh * ha * sblr, d2 = d * d;
            sc.sd = fma(d * d2, fma(d2, 1.0 / 120.0, -1.0 / 6.0), d);
            sc.cd = fma(d2, fma(d2, 1.0 / 24.0, -0.5), 1.0);
        }
        sc.s2d = 2.0 * sc.sd * sc.cd; sc.c2d = fma(-2.0 * sc.sd, sc.sd, 1.0);
        ssc(hh * ((w.v1 + ha) * sblr), w.sh, w.ch);                  // h/2 w2 of the first sub-step
        return sc;
    }

    // WHOLE_D = false (rollout_pool): a whole step taken as K == 0 leaves d0, d1 alone -- the next reader is the next control
    // step's vote, and step_head sets both from s before it (kv_d; a straight route never reads them)
    template <bool UNIFORM, bool XY = true, bool WHOLE_D = true>
    __device__ __forceinline__ void substeps(double a, double sblr, Work& w) const {
        const double ha = hh * a;
        const StepConst sc = step_const(a, sblr, w);
        // UNIFORM: kv is a scalar (one scenario per wave) and the straight-route test is hoisted; otherwise (emit: one
        // scenario per lane) the whole-step decisions are taken by votes over the active lanes -- the variants are
        // bit-identical where they apply
        if (UNIFORM && kv == 0.0) {
            run<1, XY, WHOLE_D>(sc, w);
            return;
        }
        {   // the whole control step: |travel| <= 2 dt (|v| + dt |a|)   (a straight route's d0, d1 are -inf: clear)
            const double m = (2.0 * dt) * (fabs(w.v1) + dt * fabs(a));
            const bool clear = (w.d0 + m < 0.0) | (w.d1 - m > 0.0);
            // inside the arc the travel is v / (1 - K ey) per unit time: the factor 2 of the bound holds while |K ey| < 1/2 at
            // every stage (|ey| moves by at most m / 2 within the step) -- a candidate metres off the road votes "general"
            const bool inside = (w.d0 - m > 0.0) & (w.d1 + m < 0.0) & (fabs(kv) * (fabs(w.ey) + 0.5 * m) < 0.5);
            if (__all(clear)) {
                run<1, XY, WHOLE_D>(sc, w);
                return;
            }
            if (__all(inside)) {
                run<2, XY>(sc, w);
                return;
            }
        }
        if (!UNIFORM) {                        // lanes of different scenarios rarely agree sub-step by sub-step
            run<0, XY>(sc, w);
            return;
        }
        for (int j = 0; j < nrk(); ++j) {
            // travel bound of this sub-step: |o| <= h |ds| <= 2 h (|v| + |h a|)
            const double m = (2.0 * h) * (fabs(w.v1) + 2.0 * fabs(ha));
            const bool clear = (w.d0 + m < 0.0) | (w.d1 - m > 0.0);
            const bool inside = (w.d0 - m > 0.0) & (w.d1 + m < 0.0) & (fabs(kv) * (fabs(w.ey) + 0.5 * m) < 0.5);
            if (__all(clear)) substep<1, XY>(sc, w);
            else if (__all(inside)) substep<2, XY>(sc, w);
            else substep<0, XY>(sc, w);
        }
    }
};

// ---------------------------------------------------------------------------------------
// one pass over ONE candidate per lane
// ---------------------------------------------------------------------------------------
// CAND = CAND_LATTICE / CAND_RAMP_HOLD: generated controls, input box / rate limits hold by construction;
// CAND_TABLE: controls come from the table and are checked.  Without ROLL_BOOK (emit) cost and verdicts are skipped.
// ROLL_EARLY_EXIT (search): the unit stops once every candidate of the wave has failed a verdict; then only "failed" is
// reported (vout != 0), the verdict bits are those found so far.  (The options: igt_roll_options.h.)
// Steering angle of step k for the generated families whose steering does not depend on the rolled state.
template <int CAND>
__device__ __forceinline__ double steer_next(const KP& P, const Scenario<double>& S, int k, double ddf, double df) {
    if (CAND == CAND_LATTICE) return clampd(df + ddf, -P.df_max, P.df_max);
    double ba, bdf;                                                   // CAND_RAMP_HOLD
    ramp_base<double>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
    const double tdf = clampd(bdf + ddf, -P.df_max, P.df_max);
    return clampd(df + clampd(tdf - df, -P.rate_df, P.rate_df), -P.df_max, P.df_max);
}
// ddf of steering column j (lattice increment / ramp-hold target offset) -- as rollout_one derives it from the candidate
template <int CAND>
__device__ __forceinline__ double steer_column(const KP& P, const Scenario<double>& S, int j) {
    if (CAND == CAND_LATTICE) return -P.rate_df + (2 * P.rate_df) * (double)j / (double)(P.G - 1);
    return S.cpar[1] + cand_m(j, P.G, P.refine_it == 0) * S.cpar[3];
}
// (sin, cos) of the slip angle beta = atan(r tan df), r = l_r/(l_f+l_r):  cos = c/n, sin = r s/n, n = sqrt(c^2 + r^2 s^2)
template <int CAND>
__device__ __forceinline__ void slip_trig(const KP& P, double lr_ratio, double df, double& sb, double& cb) {
    double sdf, cdf;
    if (CAND != CAND_TABLE && P.df_small) sincos_kernel(df, sdf, cdf);       // |df| <= df_max < pi/4
    else sincos_reduced(df, sdf, cdf);
    const double n = rsq_nr(fma((lr_ratio * lr_ratio) * sdf, sdf, cdf * cdf));   // argument in [r^2, 1]
    cb = cdf * n;
    sb = lr_ratio * sdf * n;
}
// Steering table of one search unit (lattice, ramp-hold): the lanes of a 64-candidate steering slice share G/W steering
// columns, each rolled by 64 W/G lanes with the same (df_k, sin beta_k, cos beta_k) -- ~50 instructions per lane and
// step that depend on nothing but the column.  The unit's wave lays the columns out once in LDS, [k][column][df, sin,
// cos] (the angles sequentially on one lane per column -- the recursion is the candidates' own -- then the trigonometry
// of all entries in parallel), with the same functions the untabulated roll-out calls: the same bits.
constexpr int STAB_MAX_ENTRIES = STEER_TABLE_MAX_ENTRIES;        // columns x N per unit (C = 256: 4 x 20, N = 40: 160; C = 64: 8 x 40)
template <int CAND>
__device__ __forceinline__ void fill_steer_table(const KP& P, const Scenario<double>& S, int nj, int r_first, int lane,
                                                 double lr_ratio, double* __restrict__ stab) {
    if (lane < nj) {                                                              // nj columns from rank r_first on (< G)
        const int r = r_first + lane;
        const int j = (r & 1) ? P.G / 2 - 1 - (r >> 1) : P.G / 2 + (r >> 1);      // unit_candidate's column order
        const double ddf = steer_column<CAND>(P, S, j);
        double df = S.df_prev;
        for (int k = 0; k < P.N; ++k) {
            df = steer_next<CAND>(P, S, k, ddf, df);
            stab[(k * nj + lane) * 3] = df;
        }
    }
    __syncthreads();
    for (int e = lane; e < nj * P.N; e += 64) {
        double sb, cb;
        slip_trig<CAND>(P, lr_ratio, stab[e * 3], sb, cb);
        stab[e * 3 + 1] = sb;
        stab[e * 3 + 2] = cb;
    }
    __syncthreads();
}
// Steering table of a pool (rollout_pool without checkpoint slots): all G columns, [k][column][df, sblr, sdb, cdb] -- what the
// pooled control step reads of the column and nothing else.  sin beta_k / l_r and the rotation by beta_k - beta_k-1 depend on
// (column, k) alone; they are formed here once, by the statements step_head / step_tail run per lane and step on the same
// operands ((sin, cos)(beta_-1) = (0, 1), as a fresh candidate carries them), so the same bits.  (sin, cos)(beta_k) pass
// through slots 1, 2 on the way: the entries are finished from the last 64 down, each from its own pair and the pair one
// step earlier (nj entries below it), which no later trip has rewritten yet.
constexpr int POOL_STAB_FIELDS = 4;
template <int CAND>
__device__ __forceinline__ void fill_pool_table(const KP& P, const Scenario<double>& S, int nj, int lane, double lr_ratio,
                                                double* __restrict__ stab) {
    constexpr int F = POOL_STAB_FIELDS;
    if (lane < nj) {
        const int j = (lane & 1) ? P.G / 2 - 1 - (lane >> 1) : P.G / 2 + (lane >> 1);      // unit_candidate's column order
        const double ddf = steer_column<CAND>(P, S, j);
        double df = S.df_prev;
        for (int k = 0; k < P.N; ++k) {
            df = steer_next<CAND>(P, S, k, ddf, df);
            stab[(k * nj + lane) * F] = df;
        }
    }
    __syncthreads();
    const int ne = nj * P.N;
    for (int e = lane; e < ne; e += 64) {
        double sb, cb;
        slip_trig<CAND>(P, lr_ratio, stab[e * F], sb, cb);
        stab[e * F + 1] = sb;
        stab[e * F + 2] = cb;
    }
    __syncthreads();
    const double inv_lr = 1.0 / P.l_r;                                  // Fast64::init
    for (int base = ((ne - 1) >> 6) << 6; base >= 0; base -= 64) {
        const int e = base + lane;
        double sblr = 0.0, sdb = 0.0, cdb = 0.0;
        if (e < ne) {
            const double sb = stab[e * F + 1], cb = stab[e * F + 2];
            double sb_prev = 0.0, cb_prev = 1.0;
            if (e >= nj) { sb_prev = stab[(e - nj) * F + 1]; cb_prev = stab[(e - nj) * F + 2]; }
            sblr = sb * inv_lr;                                         // step_head
            sdb = fma(sb, cb_prev, -(cb * sb_prev));                    // step_tail
            cdb = fma(cb, cb_prev, sb * sb_prev);
        }
        __syncthreads();                                                // every pair of this trip is read
        if (e < ne) { stab[e * F + 1] = sblr; stab[e * F + 2] = sdb; stab[e * F + 3] = cdb; }
    }
    __syncthreads();
}

// ---- the incumbent bound (search, progress cost; used by the tracking family, whose candidates hardly ever fail a verdict) ----
// A candidate's cost is  J = (non-negative stage terms, mpc.py:361-364) - (s_N - s_0)  (mpc.py:372), and the progress still to
// come after step k is bounded by the speed profile of the candidate's own acceleration row, which depends on nothing else:
// every RK4 stage derivative is  ds = v cos(.) / (1 - K ey) <= |v| / (1 - |K| |ey|),  the stage speeds of a control step lie
// between v_k and v_k+1, so  s_k+1 - s_k <= lam dt max(|v_k|, |v_k+1|)  with lam = 1 when the scenario cannot meet its arc within
// the horizon (K == 0 at every stage argument) and 1 / (1 - |kv| ey_b) else, ey_b bounding |ey| at any stage of a candidate that
// is feasible at every node (|ey_k| <= ey_lim + tol, mpc.py:296-299; it moves by at most |v| per unit time in between).  Hence
//     LB_k = J_k - (s_k - s_0) - rem_k,   rem_k = lam dt sum_{k' >= k} max(|v_k'|, |v_k'+1|)
// is a lower bound of the final cost of a candidate that ends up feasible, and one with LB_k > J_inc -- the final cost of a
// FEASIBLE candidate of the same scenario and the same pass, left by a unit that has finished (igt_kernels_f64.hip:
// search_unit64 publishes with an atomic min, units run highest acceleration rows first) -- cannot win and cannot tie: it is
// marked lost.  The winner is never among them, so cost / arg-min / trajectory are what they were, bit for bit; only HOW MANY
// steps a unit rolls depends on which incumbents it saw (tools/bound_prune_probe.py: 0.84 -> 0.46 of the wave-steps).
// (VIOL_PRUNED, cost_key / cost_of_key, progress_slack: igt_device.h -- the float path prunes the same way)

// ROLL_NO_XY (search, decided per unit by obstacles_out_of_reach): x, y are neither integrated nor judged -- no candidate
// that holds the speed box can come within d_min of any forecast position, and one that does not is infeasible already.
// inc (search, CAND_TRACK, progress cost; may be null): the scenario's incumbent key, see above.
// ---- horizon checkpoints (ROLL_LEAVE_CKPT, ROLL_RESUME): the winner's trajectory in pieces ----
// emit rolls the winner again (keeping 147 state values per candidate alive in the search would cost more), and one roll-out is
// a serial chain: 51 us at N = 20, all of it exposed when solves do not overlap.  The search pass therefore leaves, at the three
// steps k = i N / 4, what a roll-out needs to RESUME there exactly: (s, ey, epsi), the carried pair (sin, cos)(epsi + beta_k-1)
// and -- tracking family, whose steering is a feedback on the rolled state -- (df_k-1, sin beta_k-1, cos beta_k-1); everything
// else of the state at node k is a function of the candidate alone (a and v: the row's recurrence; df of the lattice / ramp-hold /
// table families: the column's) and is replayed.  ROLL_LEAVE_CKPT (search): every lane writes its values to its LDS slots `ck`
// (field-major, stride 64: igt_kernels_f64.hip search_unit64 copies the unit winner's to HBM).  ROLL_RESUME (emit_seg_f64_kernel):
// rolls steps [seg_k0, seg_k1) from the record `ck` (stride 1) of the checkpoint at seg_k0 -- the same statements on the same
// numbers, so the four pieces are the unsegmented roll-out bit for bit.  x, y, psi feed nothing back and are rolled on their own
// from the controls (cartesian_rows below).
constexpr int CK_FIELDS = 8, CK_PARTS = 4;                      // record: s ey epsi s1 c1 [df sb cb]; pieces of the horizon
constexpr int ck_fields(int cand) { return cand == CAND_TRACK ? 8 : 5; }                   // fields the family writes of a record
__host__ __device__ inline int ckpt_step(int N, int i) { return (i * N) / CK_PARTS; }      // first step of piece i

// ---- the rectangle (OBCA) collision verdict (ROLL_BOX; igt_solve_batch_box_f64 / igt_rollout_batch_box_f64) ----
// The reference's 'obca' mode (mpc.py:211-221) certifies with dual variables that the ego rectangle (centre p, heading psi) and
// an obstacle rectangle (centre q, heading phi, same half extents h) are at least d_box + 1e-6 apart.  A shooting solver judges
// the distance itself: signed gap = rectangle-to-rectangle distance, or minus the penetration depth when they overlap, and
// g = d_box + 1e-6 - gap is violated where g > tol (include/igtmpc.h has the definition, tests/box_collision_restated.py
// restates it).  Centres at least dsafe + 2 |h| apart are clear -- the gate, the only thing most pairs pay for.
//
// (q, cos phi, sin phi) of an (obstacle, node) is the same for all 64 lanes of a unit, and a libm-grade sincos of phi per pair,
// lane and step would cost more than the control step: the unit's wave lays them out once in LDS, lanes on different (o, k),
// and the step loop reads them by same-address (broadcast) ds_reads -- no bank conflict, no register held across the loop, no
// kernel argument more (the search kernels spill scalar registers as it is).  Chosen over a prelude kernel with scalar loads:
// the box solve stays one launch per pass without workspace beyond the partials, and the table costs a unit at most four
// sincos per lane against N control steps.
// A non-finite coordinate or heading (|phi| beyond 1e6 counts: sincos_reduced's domain) makes the node no constraint: the entry
// is moved out of every gate.
constexpr double BOX_NOWHERE = 1.0e150;      // its square is finite and beyond any gate
__device__ __forceinline__ void fill_box_table(const KP& P, const BoxModel& M, const double* __restrict__ pose, int lane,
                                               double* __restrict__ tab) {
    if (lane == 0) { tab[0] = M.h0; tab[1] = M.h1; tab[2] = M.dsafe; tab[3] = M.gate2; }
    for (int e = lane; e < P.n_obs * P.N; e += 64) {                  // <= BOX_TAB_MAX_ENTRIES (igt_create: n_obs, N)
        const int o = e / P.N, k = e - o * P.N + 1;
        const double* r = pose + (size_t)o * 3 * (P.N + 1) + k;      // pose [n_obs, 3, N+1]: x, y, heading
        double qx = r[0], qy = r[P.N + 1];
        const double phi = r[2 * (P.N + 1)];
        double sq = 0.0, cq = 1.0;
        if (fabs(qx) < 1.79e308 && fabs(qy) < 1.79e308 && fabs(phi) <= 1.0e6) sincos_reduced(phi, sq, cq);
        else { qx = BOX_NOWHERE; qy = 0.0; }
        double* t = tab + BOX_TAB_HEADER + e * BOX_TAB_FIELDS;
        t[0] = qx; t[1] = qy; t[2] = cq; t[3] = sq;
    }
    __syncthreads();
}
// obstacles_out_of_reach (igt_device.h) for the rectangles: dsafe + 2 |h| in place of d_min, the poses' layout
__device__ __forceinline__ bool box_out_of_reach(const KP& P, const Scenario<double>& S, const BoxModel& M,
                                                 const double* __restrict__ pose, int lane) {
    const double reach = (fmax(fabs(P.v_min), fabs(P.v_max)) + fmax(fabs(P.a_min), fabs(P.a_max)) * P.dt) * (P.N * P.dt) + 1.0;
    const double lim = sqrt(M.gate2) + reach, lim2 = lim * lim;
    bool near = false;
    for (int e = lane; e < P.n_obs * P.N; e += 64) {
        const int o = e / P.N, k = e - o * P.N + 1;
        const double dx = S.x0[0] - pose[(o * 3 + 0) * (P.N + 1) + k], dy = S.x0[1] - pose[(o * 3 + 1) * (P.N + 1) + k];
        near |= !(dx * dx + dy * dy > lim2);                      // NaN counts as near: the table sorts it out
    }
    return !__any(near);
}
// signed gap of two rectangles of half extents (h0, h1): (dx, dy) = q - p, (sp, cp) = (sin, cos) psi, (sq, cq) = (sin, cos) phi
__device__ __forceinline__ double box_gap(double h0, double h1, double dx, double dy, double sp, double cp, double sq, double cq) {
    // t = R(psi)^T (q - p): the obstacle's centre in the ego's frame; u = R(phi)^T (p - q): the roles swapped; theta = phi - psi
    const double t0 = fma(cp, dx, sp * dy), t1 = fma(cp, dy, -(sp * dx));
    const double u0 = -fma(cq, dx, sq * dy), u1 = -fma(cq, dy, -(sq * dx));
    const double ct = fma(cq, cp, sq * sp), st = fma(sq, cp, -(cq * sp));
    const double c = fabs(ct), s = fabs(st);
    // separating axes: the four depths, the extents h0 + h0 c + h1 s and h1 + h0 s + h1 c being the same in either frame
    const double e0 = fma(h1, s, fma(h0, c, h0)), e1 = fma(h1, c, fma(h0, s, h1));
    const double depth = fmin(fmin(e0 - fabs(t0), e1 - fabs(t1)), fmin(e0 - fabs(u0), e1 - fabs(u1)));
    if (depth > 0.0) return -depth;                               // overlap: minus the penetration depth
    // apart: the closest pair of points has a vertex of one rectangle at one end -- the eight vertices, each in the other's
    // frame, where its distance to the rectangle is |max(|v| - h, 0)|
    const double ax = h0 * ct, ay = h0 * st, bx = h1 * st, by = h1 * ct;
    double m = (double)INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double a = (i & 1) ? -1.0 : 1.0, b = (i & 2) ? -1.0 : 1.0;
        const double vx = fma(-b, bx, fma(a, ax, t0)), vy = fma(b, by, fma(a, ay, t1));       // t + R(theta) (a h0, b h1)
        const double wx = fma(b, bx, fma(a, ax, u0)), wy = fma(b, by, fma(-a, ay, u1));       // u + R(-theta) (a h0, b h1)
        const double ex = fmax(fabs(vx) - h0, 0.0), ey = fmax(fabs(vy) - h1, 0.0);
        const double fx = fmax(fabs(wx) - h0, 0.0), fy = fmax(fabs(wy) - h1, 0.0);
        m = fmin(m, fmin(fma(ex, ex, ey * ey), fma(fx, fx, fy * fy)));
    }
    return sqrt(m);
}
// The verdict of state k >= 1 against every obstacle.  tab: fill_box_table's.  (s2, c2) = (sin, cos)(psi_k + beta_k-1) as the
// roll-out carries it when state k is judged, (sbp, cbp) = (sin, cos)(beta_k-1): turned back by beta_k-1 they are the ego's
// (sin, cos) psi_k -- no transcendental.  The gate comes first, under a wave vote: a wave with no lane inside pays the
// difference, two products and a compare per pair.  A lane outside the gate folds nothing whatever its neighbours do, so the
// vote changes no answer; a NaN position is inside no gate (the non-finite verdict of horizon_end reports it).
template <bool LEAN>
__device__ __forceinline__ void box_collision(const KP& P, const double* __restrict__ tab, int k, double x, double y, double s2,
                                              double c2, double sbp, double cbp, double& gmax, unsigned& viol) {
    const double gate2 = tab[3];
    for (int o = 0; o < P.n_obs; ++o) {
        const double* e = tab + BOX_TAB_HEADER + (o * P.N + (k - 1)) * BOX_TAB_FIELDS;
        const double dx = e[0] - x, dy = e[1] - y;
        const bool in = fma(dx, dx, dy * dy) < gate2;
        if (__any(in)) {
            const double sp = fma(s2, cbp, -(c2 * sbp)), cp = fma(c2, cbp, s2 * sbp);
            const double g = tab[2] - box_gap(tab[0], tab[1], dx, dy, sp, cp, e[3], e[2]);
            if (in) {
                if (LEAN) gmax = fmax(gmax, g);
                else if (g > P.tol) viol |= VIOL_COLLISION;
            }
        }
    }
}

// What one lane carries from control step to control step (rollout_one, rollout_pool): the state, the candidate's control
// recurrence, the running cost and verdicts, the carried (sin, cos) pairs, the checkpoint cursor and the incumbent bound.
template <class FP>
struct LaneRoll {
    double x, y, s, ey, ep, v, psi;
    double a, df, da, ddf, J, gmax;
    unsigned viol;
    typename FP::Work w;
    double cb_prev, sb_prev;        // (sin, cos)(beta_k-1)
    double sb, cb, sblr;            // of step k: left by step_head for step_tail
    double trk_sb, trk_cb;
    bool trk_followed;
    int ck_q, ck_k;                 // next checkpoint and its step (search; -1: none)
    double rem, jcut, seg_scale;
};

// What a build is, from (CAND, options, Sink): the options by name and the constants derived from them, in one place.
template <int CAND, unsigned O, class Sink>
struct Roll {
    static constexpr bool BOOK = (O & ROLL_BOOK) != 0, UNIFORM = (O & ROLL_UNIFORM) != 0, EARLY_EXIT = (O & ROLL_EARLY_EXIT) != 0;
    static constexpr bool STAB = (O & ROLL_STEER_TABLE) != 0, XY = !(O & ROLL_NO_XY), STEPTAB = (O & ROLL_STEP_TABLE) != 0;
    static constexpr bool LEAVE_CKPT = (O & ROLL_LEAVE_CKPT) != 0, RESUME = (O & ROLL_RESUME) != 0;
    static constexpr bool EY_FOLDED = (O & ROLL_EY_FOLDED) != 0, WHOLE_D = !(O & ROLL_PART_D);
    static constexpr bool BOX = (O & ROLL_BOX) != 0;            // the rectangle verdict (box_collision) in place of the circle's
    static constexpr bool LEAN = roll_lean(O), BOUND = roll_bound(CAND, O);
    static constexpr bool KEEP_PSI = Sink::kKeepsStates;        // psi feeds nothing back (search: dead code)
    static constexpr int CKF = ck_fields(CAND);
    static_assert(roll_supported(O), "ROLL_RESUME with ROLL_LEAVE_CKPT, or ROLL_STEP_TABLE without ROLL_STEER_TABLE");
    static_assert(!STEPTAB || (CAND == CAND_LATTICE && !LEAVE_CKPT && !RESUME && !Sink::kKeepsStates),
                  "the pool's table: search only, nothing resumes from or records (sin, cos)(beta)");
};
// the control increments of a generated candidate: (da, ddf) of the lattice (oracle candidates_lattice), the
// target OFFSETS from the base sequence of the ramp-hold and tracking families (igt_device.h cand_m, ramp_base; tracking: ddf is
// the slip-angle offset of the steering feedback, track_steer)
template <int CAND>
__device__ __forceinline__ void cand_increments(const KP& P, const Scenario<double>& S, int cidx, double& da, double& ddf) {
    if (CAND == CAND_LATTICE) {
        const int i = cidx / P.G, j = cidx - i * P.G;
        da = -P.rate_a + (2 * P.rate_a) * (double)i / (double)(P.G - 1);
        ddf = steer_column<CAND>(P, S, j);
    } else if (CAND == CAND_RAMP_HOLD || CAND == CAND_TRACK) {
        const int i = cidx / P.G, j = cidx - i * P.G;
        da = S.cpar[0] + cand_m(i, P.G, P.refine_it == 0) * S.cpar[2];
        ddf = S.cpar[1] + cand_m(j, P.G, P.refine_it == 0) * S.cpar[3];
    }
}
// The controls of step k from those of step k - 1 where they are a function of the candidate alone (lattice, ramp-hold, table;
// no steering table): the replay of a resumed piece and StepControls.  The statements are step_head's, which keeps its own
// (with the table reads, the table family's verdicts and the tracking family): routed through here, two kernels came out with
// their instructions in another order (profiles/rollout_options_identity.txt).
template <int CAND>
__device__ __forceinline__ void control_step(const KP& P, const Scenario<double>& S, int k, int cidx, const double* __restrict__ table,
                                             double da, double ddf, double& a, double& df) {
    if (CAND == CAND_LATTICE) {
        a = clampd(a + da, P.a_min, P.a_max);
        df = steer_next<CAND>(P, S, k, ddf, df);
    } else if (CAND == CAND_RAMP_HOLD) {
        double ba, bdf;
        ramp_base<double>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
        const double ta = clampd(ba + da, P.a_min, P.a_max);
        a = clampd(a + clampd(ta - a, -P.rate_a, P.rate_a), P.a_min, P.a_max);
        df = steer_next<CAND>(P, S, k, ddf, df);
    } else {
        a = table[((size_t)cidx * 2 + 0) * P.N + k];
        df = table[((size_t)cidx * 2 + 1) * P.N + k];
    }
}

// The body of one control step k, in two pieces around the point where a search wave may leave early (rollout_one) and a
// pooled lane retires a candidate that failed (rollout_pool): step_head -- checkpoint, controls of step k, slip trigonometry,
// bookkeeping of state k and its verdicts, the incumbent bound -- returns whether the candidate is lost; step_tail -- the
// collision check of state k, the rotation of the carried pairs, the sub-steps -- takes the lane to state k + 1.  Every
// roll-out of the float64 path runs these statements, so whatever runs them gives the same bits.  Both halves of a step take
// the same option word O (Roll<CAND, O, Sink> names what it switches on and derives LEAN, BOUND, KEEP_PSI, CKF).  stab: the
// lane's steering column of the table (entry k at stab[k * stab_stride]); CAND_TABLE: the lane's control sequence (see the
// table branch).  ROLL_STEP_TABLE: the column is one of fill_pool_table's -- sblr comes from the table, step_tail reads the
// rotation there, and (sin, cos)(beta_k), (sin, cos)(beta_k-1) are not carried by the lane at all.  ROLL_EY_FOLDED: the pool
// folds |ey_k| - ey_lim where it decides whether the lane keeps its candidate, at the end of step k - 1 (at the refill for
// state 0); it is not folded a second time here.
template <int CAND, unsigned O, class FP, class Sink>
__device__ __forceinline__ bool step_head(const KP& P, const Scenario<double>& S, const FP& fp, LaneRoll<FP>& L, int k, int cidx,
                                          const double* __restrict__ table, const double* __restrict__ cinf, Sink& sink,
                                          const double* __restrict__ stab, int stab_stride, const unsigned long long* inc,
                                          double* ck, bool rows_judged, bool kv_d) {
    typedef Roll<CAND, O, Sink> R;
    constexpr bool BOOK = R::BOOK, LEAN = R::LEAN, STAB = R::STAB, STEPTAB = R::STEPTAB;
    if (R::LEAVE_CKPT && k == L.ck_k) {          // node k: what a roll-out needs to resume here
        double* c = ck + (size_t)(L.ck_q - 1) * R::CKF * 64;
        c[0] = L.s; c[64] = L.ey; c[128] = L.ep; c[192] = L.w.s1; c[256] = L.w.c1;
        if (CAND == CAND_TRACK) { c[320] = L.df; c[384] = L.sb_prev; c[448] = L.cb_prev; }
        ++L.ck_q;
        L.ck_k = L.ck_q < CK_PARTS ? ckpt_step(P.N, L.ck_q) : -1;
    }
    // ---- controls of step k
    if (CAND == CAND_LATTICE) {
        L.a = clampd(L.a + L.da, P.a_min, P.a_max);
        L.df = STAB ? stab[k * stab_stride] : steer_next<CAND>(P, S, k, L.ddf, L.df);
    } else if (CAND == CAND_RAMP_HOLD) {
        double ba, bdf;
        ramp_base<double>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
        const double ta = clampd(ba + L.da, P.a_min, P.a_max);
        L.a = clampd(L.a + clampd(ta - L.a, -P.rate_a, P.rate_a), P.a_min, P.a_max);
        L.df = STAB ? stab[k * stab_stride] : steer_next<CAND>(P, S, k, L.ddf, L.df);
    } else if (CAND == CAND_TRACK) {
        double ba, bdf;
        ramp_base<double>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
        L.a = track_accel_next(P, k, ba, L.da, L.v, L.a);
        L.df = track_steer(P, L.df, L.ey, L.ep, L.ddf, &L.trk_sb, &L.trk_cb, &L.trk_followed);
    } else {
        // STAB (polish_f64_kernel): the lane's own controls in LDS, a at stab[k * stab_stride], delta_f N entries behind
        const double an = STAB ? stab[(size_t)k * stab_stride] : table[((size_t)cidx * 2 + 0) * P.N + k];
        const double dn = STAB ? stab[(size_t)(P.N + k) * stab_stride] : table[((size_t)cidx * 2 + 1) * P.N + k];
        if (BOOK) {   // input-rate (mpc.py:301-312, u_{-1} = u_prev) and input box (mpc.py:318-321)
            if (fmax(fabs(an - L.a) - P.rate_a, fabs(dn - L.df) - P.rate_df) > P.tol) L.viol |= VIOL_RATE;
            if (fmax(fmax(P.a_min - an, an - P.a_max), fmax(-P.df_max - dn, dn - P.df_max)) > P.tol) L.viol |= VIOL_BOX_U;
        }
        L.a = an; L.df = dn;
    }
    sink.ctrl(0, k, L.a, L.df);
    double sb, cb;                               // (sin, cos)(beta), beta = atan(r tan df)
    if (STEPTAB) {
        L.sblr = stab[k * stab_stride + 1];
    } else if (STAB && (CAND == CAND_LATTICE || CAND == CAND_RAMP_HOLD)) {
        sb = stab[k * stab_stride + 1];
        cb = stab[k * stab_stride + 2];
    } else if (CAND == CAND_TRACK) {
        // a lane whose steering followed the command has beta = beta_cmd: its (sin, cos) are known already.  The other
        // lanes (rate- or box-limited) go through sincos(df); the wave skips that when no lane needs it -- which lane
        // takes which value does not depend on the vote, so search, emit and rollout-all agree bit for bit
        sb = L.trk_sb; cb = L.trk_cb;
        if (!__all(L.trk_followed)) {
            double sb2, cb2;
            slip_trig<CAND>(P, fp.lr_ratio, L.df, sb2, cb2);
            sb = L.trk_followed ? sb : sb2;
            cb = L.trk_followed ? cb : cb2;
        }
    } else {
        slip_trig<CAND>(P, fp.lr_ratio, L.df, sb, cb);
    }
    if (!STEPTAB) {
        sink.slip(0, k, sb, cb);
        L.sb = sb; L.cb = cb;
        L.sblr = sb * fp.inv_lr;
    }
    // ---- bookkeeping of state k (cost in the oracle's order: control effort, epsi^2, ey^2 -- mpc.py:361-364)
    if (BOOK) {
        L.J = L.J + P.w_u * (L.a * L.a + L.df * L.df);
        L.J = L.J + L.ep * L.ep;
        L.J = L.J + L.ey * L.ey;
        if (LEAN) {
            if (!R::EY_FOLDED) L.gmax = fmax(L.gmax, fabs(L.ey) - P.ey_lim);                  // mpc.py:296-299
            if (!rows_judged) L.gmax = fmax(L.gmax, fmax(P.v_min - L.v, L.v - P.v_max));   // mpc.py:316-317 (k < N)
        } else {
            if (fabs(L.ey) - P.ey_lim > P.tol) L.viol |= VIOL_EY;
            if (fmax(P.v_min - L.v, L.v - P.v_max) > P.tol) L.viol |= VIOL_BOX_V;
        }
        if (k == P.N - 1 && !rows_judged) L.viol |= terminal_viol(P, L.v, L.a, cinf);  // mpc.py:177-180
    }
    L.w.ey = L.ey; L.w.v1 = L.v;
    // unused on straight routes; with one scenario per lane the votes of substeps() read them on every lane
    // (a straight route's break-points are +inf: d = -inf, "clear")
    if (kv_d) { L.w.d0 = L.s - fp.b0; L.w.d1 = L.s - fp.b1; }
    if (R::BOUND && inc) {
        // the incumbent is re-read every fourth step (a unit that started before its scenario's first unit finished picks it
        // up on the way); agent scope: the units of a scenario may run on different XCDs, whose L2s are not coherent
        if ((k & 3) == 0) {
            const double ji = cost_of_key(__hip_atomic_load(inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            L.jcut = ji + 1e-9 * (1.0 + fabs(ji));
        }
        if ((L.J - (L.s - S.x0[2])) - L.rem > L.jcut) L.viol |= VIOL_PRUNED;
    }
    return (L.viol != 0) | (LEAN && L.gmax > P.tol);
}
template <int CAND, unsigned O, class FP, class Sink>
__device__ __forceinline__ void step_tail(const KP& P, const Scenario<double>& S, const FP& fp, LaneRoll<FP>& L, int k, Sink& sink,
                                          const unsigned long long* inc, const double* __restrict__ stab = nullptr,
                                          int stab_stride = 0) {
    typedef Roll<CAND, O, Sink> R;
    constexpr bool BOOK = R::BOOK, LEAN = R::LEAN, XY = R::XY, STEPTAB = R::STEPTAB;
    if constexpr (R::BOX) {                                                      // rectangles, mpc.py:211-221
        if (BOOK && XY && k >= 1) box_collision<LEAN>(P, S.obs, k, L.x, L.y, L.w.s2, L.w.c2, L.sb_prev, L.cb_prev, L.gmax, L.viol);
    } else
    if (BOOK && XY && k >= 1) {                                                  // collision, mpc.py:223-226
        for (int o = 0; o < P.n_obs; ++o) {
            const double dx = L.x - S.obs[(o * 2 + 0) * (P.N + 1) + k], dy = L.y - S.obs[(o * 2 + 1) * (P.N + 1) + k];
            const double g = P.dmin2 - (dx * dx + dy * dy);
            if (LEAN) L.gmax = fmax(L.gmax, g);
            else if (g > P.tol) L.viol |= VIOL_COLLISION;
        }
    }
    // (sin,cos)(psi + beta_k) from (psi + beta_{k-1}), and (sin,cos)(epsi + beta_k) from (epsi + beta_{k-1}): rotate by
    // beta_k - beta_{k-1}, re-normalise (first order: the pairs are within rounding of unit length)
    {
        double sdb, cdb;
        if (STEPTAB) {                                       // fill_pool_table: these statements, once per (column, k)
            sdb = stab[k * stab_stride + 2];
            cdb = stab[k * stab_stride + 3];
        } else {
            const double sb = L.sb, cb = L.cb;
            sdb = fma(sb, L.cb_prev, -(cb * L.sb_prev));
            cdb = fma(cb, L.cb_prev, sb * L.sb_prev);
        }
        rotate(L.w.s1, L.w.c1, sdb, cdb);
        const double r1 = fma(fma(L.w.s1, L.w.s1, L.w.c1 * L.w.c1), -0.5, 1.5);
        L.w.s1 *= r1; L.w.c1 *= r1;
        if (XY) {
            rotate(L.w.s2, L.w.c2, sdb, cdb);
            const double r2 = fma(fma(L.w.s2, L.w.s2, L.w.c2 * L.w.c2), -0.5, 1.5);
            L.w.s2 *= r2; L.w.c2 *= r2;
        }
        if (!STEPTAB) { L.cb_prev = L.cb; L.sb_prev = L.sb; }
    }
    L.w.acc_s = 0.0; L.w.acc_ey = 0.0; L.w.acc_ep = 0.0; L.w.acc_x = 0.0; L.w.acc_y = 0.0; L.w.acc_psi = 0.0;
    fp.template substeps<R::UNIFORM, XY, R::WHOLE_D>(L.a, L.sblr, L.w);
    L.s += L.w.acc_s; L.ey += L.w.acc_ey; L.ep += L.w.acc_ep;
    if (XY) { L.x += L.w.acc_x; L.y += L.w.acc_y; }
    if (R::KEEP_PSI) L.psi += L.w.acc_psi;
    if (R::BOUND && inc) L.rem -= L.seg_scale * fmax(fabs(L.v), fabs(fma(fp.dt, L.a, L.v)));      // this step's share of the bound is spent
    L.v = fma(fp.dt, L.a, L.v);
    const double nxt[7] = {L.x, L.y, L.s, L.ey, L.ep, L.v, L.psi};
    sink.state(0, k + 1, nxt);
}
// the bookkeeping of state N, after the last control step
template <unsigned O, class FP>
__device__ __forceinline__ void horizon_end(const KP& P, const Scenario<double>& S, LaneRoll<FP>& L, double& Jout, unsigned& vout,
                                            double& sN, double& vN) {
    constexpr bool LEAN = roll_lean(O), XY = !(O & ROLL_NO_XY);
    L.J = L.J + L.ep * L.ep;
    L.J = L.J + L.ey * L.ey;
    if (LEAN) L.gmax = fmax(L.gmax, fabs(L.ey) - P.ey_lim);
    else if (fabs(L.ey) - P.ey_lim > P.tol) L.viol |= VIOL_EY;
    if constexpr ((O & ROLL_BOX) != 0) {               // state N: the pair holds psi_N + beta_N-1
        if (XY) box_collision<LEAN>(P, S.obs, P.N, L.x, L.y, L.w.s2, L.w.c2, L.sb_prev, L.cb_prev, L.gmax, L.viol);
    } else
    for (int o = 0; XY && o < P.n_obs; ++o) {
        const double dx = L.x - S.obs[(o * 2 + 0) * (P.N + 1) + P.N], dy = L.y - S.obs[(o * 2 + 1) * (P.N + 1) + P.N];
        const double g = P.dmin2 - (dx * dx + dy * dy);
        if (LEAN) L.gmax = fmax(L.gmax, g);
        else if (g > P.tol) L.viol |= VIOL_COLLISION;
    }
    if (LEAN && L.gmax > P.tol) L.viol |= VIOL_EY;     // lean form: "some state-side verdict failed"
    if (!(fabs(L.x) < 1e300 && fabs(L.y) < 1e300 && fabs(L.s) < 1e300 && fabs(L.ey) < 1e300 && fabs(L.ep) < 1e300 &&
          fabs(L.psi) < 1e300))
        L.viol |= VIOL_NONFINITE;
    sN = L.s; vN = L.v; Jout = L.J; vout = L.viol;
}

// One candidate per lane over the horizon (ROLL_RESUME: over steps [seg_k0, seg_k1) from the record ck).  O: the build's
// options, a role of igt_roll_options.h and what the call site adds to it.  The optional inputs stay positional scalars: as
// one aggregate, by value or by reference, and behind forwarding functions that name them, they changed the order of some
// kernels' instructions (profiles/rollout_options_identity.txt).
template <int CAND, bool HI_ORDER, unsigned O, int NRK = 0, class Sink>
__device__ __forceinline__ void rollout_one(const KP& P, const Scenario<double>& S, int cidx,
                                            const double* __restrict__ table, const double* __restrict__ cinf,
                                            Sink& sink, double& Jout, unsigned& vout, double& sN, double& vN,
                                            const double* __restrict__ stab = nullptr, int stab_stride = 0,
                                            const unsigned long long* inc = nullptr, double* ck = nullptr, int seg_k0 = 0,
                                            int seg_k1 = 0, const double* __restrict__ rem_rows = nullptr) {
    typedef Roll<CAND, O, Sink> R;
    constexpr bool BOOK = R::BOOK, UNIFORM = R::UNIFORM, EARLY_EXIT = R::EARLY_EXIT, XY = R::XY, RESUME = R::RESUME;
    // search on units of live acceleration rows (igt_kernels_f64.hip accel_rows_kernel; DEV_LAUNCH_LIVE_ROWS): the speed
    // box and the terminal set read the row's (a, v) recurrence alone and were judged there, with these statements -- every lane
    // that holds a candidate holds one of a row that passed: not judged again (74 half-planes per lane at the last step)
    const bool rows_judged = BOOK && EARLY_EXIT && UNIFORM && CAND != CAND_TABLE && (P.dev & DEV_LAUNCH_LIVE_ROWS) != 0;
    typedef Fast64<HI_ORDER, NRK> FP;
    FP fp;
    fp.init(P, S.b0, S.b1, S.kv);
    LaneRoll<FP> L;
    L.x = S.x0[0]; L.y = S.x0[1]; L.s = S.x0[2]; L.ey = S.x0[3]; L.ep = S.x0[4]; L.v = S.x0[5]; L.psi = S.x0[6];
    L.a = S.a_prev; L.df = S.df_prev; L.da = 0.0; L.ddf = 0.0; L.J = 0.0; L.gmax = -1.0e300;
    // cidx < 0 (search): a lane of the unit that holds no candidate (igt_kernels_f64.hip unit_candidate) -- it rolls candidate 0
    // in step with the wave and is "lost" from the start, so it neither wins nor keeps the unit alive
    L.viol = cidx < 0 ? (unsigned)VIOL_EY : 0u;
    if (cidx < 0) cidx = 0;
    bool dead = false;
    cand_increments<CAND>(P, S, cidx, L.da, L.ddf);
    if (!RESUME || seg_k0 == 0) sink.state(0, 0, S.x0);
    L.w.d0 = L.w.d1 = 0.0;
    if (XY) sincos_reduced(S.x0[6], L.w.s2, L.w.c2);       // carried as (sin,cos)(psi + beta_k); beta_{-1} = 0
    else { L.w.s2 = 0.0; L.w.c2 = 1.0; }
    // (sin,cos)(epsi + beta_k) is carried the same way: the sub-steps turn the pair by exactly the angle epsi advances by
    // (substep(): h w2 - corr per sub-step), so after control step k-1 it holds (sin,cos)(epsi_k + beta_{k-1}) and step k
    // turns it by beta_k - beta_{k-1} -- no sincos(epsi) per control step (39 of ~460 instructions on a straight route)
    L.cb_prev = 1.0; L.sb_prev = 0.0;
    L.trk_sb = 0.0; L.trk_cb = 1.0;
    L.trk_followed = false;
    int k_first = 0, k_last = P.N;
    if (RESUME) { k_first = seg_k0; k_last = seg_k1; }
    if (RESUME && seg_k0 > 0) {
        // resume at node seg_k0: the controls' own recurrences are replayed, the state that depends on the roll-out comes from
        // the checkpoint
        for (int k = 0; k < seg_k0; ++k) {
            if (CAND == CAND_TRACK) {                  // a only: the steering comes from the record
                double ba, bdf;
                ramp_base<double>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
                L.a = track_accel_next(P, k, ba, L.da, L.v, L.a);
            } else {
                control_step<CAND>(P, S, k, cidx, table, L.da, L.ddf, L.a, L.df);
            }
            L.v = fma(fp.dt, L.a, L.v);
        }
        L.s = ck[0]; L.ey = ck[1]; L.ep = ck[2]; L.w.s1 = ck[3]; L.w.c1 = ck[4];
        if (CAND == CAND_TRACK) { L.df = ck[5]; L.sb_prev = ck[6]; L.cb_prev = ck[7]; }
        else slip_trig<CAND>(P, fp.lr_ratio, L.df, L.sb_prev, L.cb_prev);      // of df_{k0-1}: what step k0-1 left in (sb_prev, cb_prev)
    } else {
        sincos_reduced(S.x0[4], L.w.s1, L.w.c1);
    }
    L.ck_q = 1; L.ck_k = (R::LEAVE_CKPT && ck) ? ckpt_step(P.N, 1) : -1;  // next checkpoint and its step (search; none without slots)
    // incumbent bound: rem = bound of the progress still to come (the row's own (a, v) recurrence rolled ahead, the statements of
    // the loop below), jcut = incumbent + a margin far above the rounding of LB_k (1e-9: the comparison is mathematically strict)
    L.rem = 0.0; L.jcut = (double)INFINITY; L.seg_scale = 0.0;
    if (R::BOUND && inc) {
        L.seg_scale = progress_slack(P, S) * P.dt;
        if (L.seg_scale > 0.0) {
            if (rem_rows) {       // the row's sum as accel_rows_kernel left it (the statements of the loop in the other branch)
                L.rem = rem_rows[cidx / P.G];
            } else {
                double a2 = S.a_prev, v2 = S.x0[5];
                for (int k = 0; k < P.N; ++k) {
                    double ba, bdf;
                    ramp_base<double>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
                    a2 = track_accel_next(P, k, ba, L.da, v2, a2);
                    const double vn = fma(fp.dt, a2, v2);
                    L.rem += fmax(fabs(v2), fabs(vn));
                    v2 = vn;
                }
            }
            L.rem *= L.seg_scale * (1.0 + 1e-12);
        } else {
            inc = nullptr;
        }
    }

    const bool kv_d = !UNIFORM || fp.kv != 0.0;
    for (int k = k_first; k < k_last; ++k) {
        const bool lost = step_head<CAND, O>(P, S, fp, L, k, cidx, table, cinf, sink, stab, stab_stride, inc, ck, rows_judged, kv_d);
        if (BOOK && UNIFORM && EARLY_EXIT) {
            // search only: once every candidate of the slice has failed a verdict, nothing rolled further can win
            if (__all(lost) && !(P.dev & DEV_NO_EARLY_EXIT)) { dead = true; break; }
        }
        step_tail<CAND, O>(P, S, fp, L, k, sink, inc);
    }
    if (dead) {            // costs are meaningless; "failed" is what is reported
        Jout = 0.0; vout = L.viol | ((R::LEAN && L.gmax > P.tol) ? VIOL_EY : 0u); sN = 0.0; vN = 0.0;
        return;
    }
    if (BOOK) {
        horizon_end<O>(P, S, L, Jout, vout, sN, vN);
    } else {
        Jout = 0.0; vout = 0; sN = 0.0; vN = 0.0;
    }
}

// ---- the pool roll-out (search, lattice family on live rows with the whole steering table in LDS) ----
// A unit of 64 candidates leaves through the early exit only when all 64 have failed, and a lattice candidate is feasible
// rarely (5 %) and dies mostly between steps 4 and 12: a unit's wave spends much of its time issuing for lanes that are dead
// already.  Here one wave owns all n candidates of its scenario as a pool: every lane holds a candidate number, a step k of
// its own and its state; one iteration is one control step for every lane that holds a candidate, each at its own k; a lane
// whose candidate has failed a verdict by the end of its step (|ey| of the state it reached, a collision of the one it left) or
// reached k = N (horizon_end) takes the pool's next number -- numbers are handed
// out by a ballot and a prefix count from a wave-uniform cursor, no atomics (tools/refill_model.py: 0.52 -> 0.39 of the
// wave-steps on the benchmark batch).  The statements are rollout_one's (step_head / step_tail / horizon_end), so every
// candidate's cost and verdicts are the bits the units compute; the sub-step votes run over lanes at different k and may pick
// another variant than a unit's wave would -- the variants are bit-identical where they apply.
// The arg-min: the candidates that finish feasible in an iteration are reduced together with the wave's best on (Jq, c), ties
// to the lowest index -- a total order, so the winner does not depend on the order the pool is worked in.  With checkpoint slots
// (ck: the lane's column of the LDS records, SEGMODE 1) the new winner's lane copies its records to `rec` (15 doubles).
// start: POOL_START doubles of LDS for what a refill reads of the scenario (read there when a lane refills instead of held in
// registers over the whole loop: the kernel is at its 256 registers).
// tabw, tabda: POOL_TAB entries of LDS each -- what a refill needs that depends on the candidate number alone, for a window of
// POOL_TAB numbers: the candidate index and its column rank in one word (index | rank << 16), and da.  fill(base) has the
// wave lay out the window that starts at number `base` (igt_kernels_f64.hip search_pool64); it is called when the cursor first
// reaches past the window (once per item when n <= POOL_TAB, i.e. C <= 256), with the values a refill used to compute on the
// spot, so the same bits -- and a refill is a wave-uniform branch around a few LDS reads.
// O: ROLL_POOL and one of ROLL_LEAVE_CKPT -- checkpoint slots (ck, rec: emit in pieces) over the three-double table of
// fill_steer_table -- and ROLL_STEP_TABLE -- neither is touched, nothing of the checkpoint cursor is carried, and the table is
// fill_pool_table's; ROLL_NO_XY as the item decides.  Both halves of the step get this word.
// The four-double table does not fit beside the slots in the 20 KB a wave may take (eight waves per compute unit).
constexpr int POOL_START = 13, POOL_TAB = 256;
template <int CAND, bool HI_ORDER, int NRK, unsigned O, class Fill>
__device__ __forceinline__ void rollout_pool(const KP& P, const Scenario<double>& S, int n, const Fill& fill,
                                             const double* __restrict__ cinf, const double* __restrict__ stab, int stab_stride,
                                             double* ck, double* rec, double* start, unsigned* tabw, double* tabda,
                                             double& wJ, int& wC) {
    static_assert(CAND == CAND_LATTICE, "pool roll-out: the lattice family (its steering is a column of the table)");
    static_assert((O & ROLL_POOL) == ROLL_POOL && ((O & ROLL_LEAVE_CKPT) != 0) != ((O & ROLL_STEP_TABLE) != 0), "see above");
    constexpr bool XY = !(O & ROLL_NO_XY), CKPT = (O & ROLL_LEAVE_CKPT) != 0;
    constexpr int CKF = ck_fields(CAND);
    constexpr int SF = CKPT ? 3 : POOL_STAB_FIELDS;          // doubles per table entry
    typedef Fast64<HI_ORDER, NRK> FP;
    FP fp;
    fp.init(P, S.b0, S.b1, S.kv);
    NullSink sink;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the initial pairs are the scenario's: once per item instead of once per candidate
    if (lane == 0) {
        double s1_0, c1_0, s2_0 = 0.0, c2_0 = 1.0;
        sincos_reduced(S.x0[4], s1_0, c1_0);
        if (XY) sincos_reduced(S.x0[6], s2_0, c2_0);
#pragma unroll
        for (int i = 0; i < 7; ++i) start[i] = S.x0[i];
        start[7] = S.a_prev; start[8] = S.df_prev;
        start[9] = s1_0; start[10] = c1_0; start[11] = s2_0; start[12] = c2_0;
    }
    __syncthreads();
    const bool kv_d = fp.kv != 0.0;
    LaneRoll<FP> L;
    L.psi = S.x0[6];                                // psi feeds nothing back (search)
    L.da = 0.0; L.ddf = 0.0; L.trk_sb = 0.0; L.trk_cb = 1.0; L.trk_followed = false;
    L.rem = 0.0; L.jcut = (double)INFINITY; L.seg_scale = 0.0;
    int c = 0, k = 0;
    const double* lstab = stab;
    bool hold = false;
    int next = 0;                                   // the pool's cursor (wave-uniform)
    int tab_end = 0;                                // the table holds the numbers [tab_end - POOL_TAB, tab_end): none yet
    wJ = 0.0; wC = -1;
    for (;;) {
        // ---- idle lanes take the next numbers (a branch the whole wave takes or skips: most iterations refill nothing)
        const unsigned long long want = __ballot(!hold);
        if (want != 0ull && next < n) {
            // the body stays behind the wave's branch, not if-converted into the iteration.  What holds it there is visible in the
            // ISA only (profiles/r07_pool_loop_isa.txt): an s_cbranch_vccnz around the refill, no f64 division inside the loop
            __builtin_amdgcn_sched_barrier(0);
            const int cnt = __popcll(want);
            if (next + cnt > tab_end && tab_end < n) {           // the numbers handed out now reach past the window: next one
                tab_end = next + POOL_TAB;
                fill(next);
            }
            const int g = next + __popcll(want & below);
            if (!hold && g < n) {
                const int e = g - (tab_end - POOL_TAB);
                const unsigned w = tabw[e];
                L.da = tabda[e];
                c = (int)(w & 0xffffu);
                lstab = stab + (w >> 16) * SF;
                L.x = start[0]; L.y = start[1]; L.s = start[2]; L.ey = start[3]; L.ep = start[4]; L.v = start[5];
                L.a = start[7]; L.df = start[8]; L.J = 0.0; L.viol = 0u;
                L.gmax = fmax(-1.0e300, fabs(L.ey) - P.ey_lim);         // the |ey| verdict of state 0 (step_head EY_FOLDED)
                L.w.d0 = L.w.d1 = 0.0;
                L.w.s1 = start[9]; L.w.c1 = start[10]; L.w.s2 = start[11]; L.w.c2 = start[12];
                if (CKPT) {
                    L.cb_prev = 1.0; L.sb_prev = 0.0;
                    L.ck_q = 1; L.ck_k = ck ? ckpt_step(P.N, 1) : -1;
                }
                k = 0; hold = true;
            }
            next += cnt;
        }
        if (__ballot(hold) == 0ull) break;
        // ---- control step k for every lane that holds a candidate; it retires a candidate whose state k + 1 < N fails already,
        // and one that reached state N after the bookkeeping of the end of the horizon
        bool fin = false;
        double Jq = 0.0;
        if (hold) {
            const bool rows_judged = true;              // a pool is of live rows
            step_head<CAND, O>(P, S, fp, L, k, c, nullptr, cinf, sink, lstab, stab_stride, nullptr, ck, rows_judged, kv_d);
            step_tail<CAND, O>(P, S, fp, L, k, sink, nullptr, lstab, stab_stride);
            ++k;
            // state k is complete.  A candidate that fails its |ey| verdict, or failed the collision verdict of state k - 1
            // (step_tail), can never finish feasible -- gmax only grows -- and gives up its lane now, not after one more step.
            // The fold is step_head's own for state k, made here once (EY_FOLDED); step_head's verdict is not read: all it
            // can report in a pool is gmax > tol, which this test sees at the end of the same step.  State N is horizon_end's,
            // and so is a candidate that reaches it with a failed verdict (N = 1): it finishes infeasible.
            if (k < P.N) L.gmax = fmax(L.gmax, fabs(L.ey) - P.ey_lim);                          // mpc.py:296-299
            if (k < P.N && L.gmax > P.tol) {
                hold = false;
            } else if (k == P.N) {
                double J, sN, vN;
                unsigned viol;
                horizon_end<O>(P, S, L, J, viol, sN, vN);
                Jq = J - (sN - start[2]);                      // mpc.py:372 (start[2] = x0[2])
                fin = viol == 0 && fabs(Jq) < 1.79e308;        // finite_d
                hold = false;
            }
        }
        // ---- feasible candidates that finished: reduced with the wave's best (the units' butterfly and tie rule)
        // only when one of them can replace the wave's best: the order on (Jq, c) is total, so the minimum over the finishers
        // beats (wJ, wC) exactly when some finisher does -- same winner, same lane copying its records
        if (__ballot(fin && (wC < 0 || Jq < wJ || (Jq == wJ && c < wC))) != 0ull) {
            double bJ = Jq;
            int bC = fin ? c : -1;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double oJ = __shfl_xor(bJ, off, 64);
                const int oC = __shfl_xor(bC, off, 64);
                const bool take = (oC >= 0) && (bC < 0 || oJ < bJ || (oJ == bJ && oC < bC));      // wave_argmin (igt_device.h) written out
                if (take) { bJ = oJ; bC = oC; }
            }
            bJ = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(bJ)), __builtin_amdgcn_readfirstlane(__double2loint(bJ)));
            bC = __builtin_amdgcn_readfirstlane(bC);
            if (wC < 0 || bJ < wJ || (bJ == wJ && bC < wC)) {
                wJ = bJ; wC = bC;
                if (CKPT && ck && fin && c == bC) {           // the new winner's checkpoints, [q][field]
#pragma unroll
                    for (int q = 0; q < CK_PARTS - 1; ++q)
#pragma unroll
                        for (int f = 0; f < CKF; ++f) rec[q * CKF + f] = ck[(size_t)(q * CKF + f) * 64];
                }
            }
        }
    }
}

// The Cartesian rows x, y, psi of a trajectory from its controls alone (emit_seg_f64_kernel): they feed nothing back
// (frenet.py:84-90), and what they read -- the stage speeds, the psi offsets, (sin, cos)(psi + beta) carried by rotation --
// depends on (a_k, sin beta_k, cos beta_k) only.  The statements are rollout_one's: the pair is turned and re-normalised as
// there, the step's constants come from step_const, and the sub-steps are substep<1, true> itself (its Frenet part reads
// nothing of the Cartesian one and is dead code here) -- so x, y, psi come out bit for bit as in the full roll-out, whatever
// sub-step variant that took (the variants differ in the Frenet part only).
// ctl(k, a, sb, cb): the controls of step k -- read back from where the Frenet pieces left them (tracking family: the steering is
// theirs to decide) or generated on the spot (the families whose controls are a function of the candidate alone: StepControls);
// X, Y, PSI: [N+1] outputs with element stride `xs` (node 0 is written by the caller).
template <bool HI_ORDER, int NRK, class Ctl>
__device__ __forceinline__ void cartesian_rows(const KP& P, double x, double y, double psi, double v, Ctl& ctl,
                                               double* X, double* Y, double* PSI, int xs) {
    typedef Fast64<HI_ORDER, NRK> FP;
    FP fp;
    fp.init(P, (double)INFINITY, (double)INFINITY, 0.0);
    typename FP::Work w;
    w.d0 = w.d1 = 0.0; w.s1 = 0.0; w.c1 = 1.0; w.ey = 0.0;
    sincos_reduced(psi, w.s2, w.c2);
    double cb_prev = 1.0, sb_prev = 0.0;
    for (int k = 0; k < P.N; ++k) {
        double a, sb, cb;
        ctl(k, a, sb, cb);
        const double sblr = sb * fp.inv_lr;
        w.v1 = v;
        {
            const double sdb = fma(sb, cb_prev, -(cb * sb_prev));
            const double cdb = fma(cb, cb_prev, sb * sb_prev);
            rotate(w.s2, w.c2, sdb, cdb);
            const double r2 = fma(fma(w.s2, w.s2, w.c2 * w.c2), -0.5, 1.5);
            w.s2 *= r2; w.c2 *= r2;
            cb_prev = cb; sb_prev = sb;
        }
        w.acc_s = 0.0; w.acc_ey = 0.0; w.acc_ep = 0.0; w.acc_x = 0.0; w.acc_y = 0.0; w.acc_psi = 0.0;
        const typename FP::StepConst sc = fp.step_const(a, sblr, w);
        fp.template run<1, true>(sc, w);
        x += w.acc_x; y += w.acc_y; psi += w.acc_psi;
        v = fma(fp.dt, a, v);
        X[(size_t)(k + 1) * xs] = x; Y[(size_t)(k + 1) * xs] = y; PSI[(size_t)(k + 1) * xs] = psi;
    }
}

// The controls of the families whose candidates do not read the rolled state (lattice, ramp-hold, table), step by step, with
// (sin, cos)(beta_k): rollout_one's statements for them (its control block and slip_trig), for the wave that rolls the Cartesian
// rows beside the Frenet pieces.
template <int CAND>
struct StepControls {
    const KP& P;
    const Scenario<double>& S;
    const double* table;
    int cidx;
    double a, df, da, ddf, lr_ratio;
    __device__ __forceinline__ StepControls(const KP& P_, const Scenario<double>& S_, int c, const double* t)
        : P(P_), S(S_), table(t), cidx(c), a(S_.a_prev), df(S_.df_prev), da(0.0), ddf(0.0), lr_ratio(P_.lr_ratio) {
        cand_increments<CAND>(P, S, cidx, da, ddf);
    }
    __device__ __forceinline__ void operator()(int k, double& a_out, double& sb, double& cb) {
        control_step<CAND>(P, S, k, cidx, table, da, ddf, a, df);
        slip_trig<CAND>(P, lr_ratio, df, sb, cb);
        a_out = a;
    }
};

}  // namespace f64
}  // namespace igt
