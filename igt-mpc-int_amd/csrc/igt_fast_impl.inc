// igt_fast_impl.inc -- the vector-width-dependent part of igt_fast.h; included once per width (IGT_NV = 2: two
// candidates per lane, the search / rollout-all build; IGT_NV = 1: one candidate per lane, the emit build).  The
// operation sequence per candidate is the same in both, so they agree bit for bit (-ffp-contract=off).
typedef float f2 __attribute__((ext_vector_type(IGT_NV)));   // the lane's IGT_NV candidates side by side
constexpr int NV = IGT_NV;

__device__ __forceinline__ f2 splat(float x) { f2 r = x; return r; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 rcp2(f2 x) {
    f2 r;
#pragma unroll
    for (int q = 0; q < NV; ++q) r[q] = __builtin_amdgcn_rcpf(x[q]);
    return r;
}
__device__ __forceinline__ f2 clamp01(f2 x) {
    f2 r;
#pragma unroll
    for (int q = 0; q < NV; ++q) r[q] = __builtin_amdgcn_fmed3f(x[q], 0.0f, 1.0f);
    return r;
}

// |d| <= ~0.12: sin to d^5, cos to d^4 (truncation 7e-11 / 4e-9)
__device__ __forceinline__ void small_sincos2(f2 d, f2& sd, f2& cd) {
    const f2 d2 = d * d;
    const f2 p = fma2(d2, splat(1.0f / 120.0f), splat(-1.0f / 6.0f));
    sd = fma2(d * d2, p, d);
    const f2 q = fma2(d2, splat(1.0f / 24.0f), splat(-0.5f));
    cd = fma2(d2, q, splat(1.0f));
}
// half-step offsets |d| <= h/2 * |rate| (<= 0.03 for any feasible state at h = 0.025): sin to d^3, cos to d^2;
// the dropped terms d^5/120 and d^4/24 are below 3e-8 there
__device__ __forceinline__ void tiny_sincos2(f2 d, f2& sd, f2& cd) {
    const f2 d2 = d * d;
    sd = fma2(d * d2, splat(-1.0f / 6.0f), d);
    cd = fma2(d2, splat(-0.5f), splat(1.0f));
}
// |d| <= 0.5 variant (coarser discretisations): two more terms
__device__ __forceinline__ void small_sincos2_hi(f2 d, f2& sd, f2& cd) {
    const f2 d2 = d * d;
    f2 p = fma2(d2, splat(-1.0f / 5040.0f), splat(1.0f / 120.0f));
    p = fma2(d2, p, splat(-1.0f / 6.0f));
    sd = fma2(d * d2, p, d);
    f2 q = fma2(d2, splat(1.0f / 40320.0f), splat(-1.0f / 720.0f));
    q = fma2(d2, q, splat(1.0f / 24.0f));
    q = fma2(d2, q, splat(-0.5f));
    cd = fma2(d2, q, splat(1.0f));
}

__device__ __forceinline__ void rotate2(f2& s, f2& c, f2 sd, f2 cd) {
    const f2 s_ = fma2(s, cd, c * sd);
    const f2 c_ = fma2(c, cd, -(s * sd));
    s = s_; c = c_;
}

template <bool HI_ORDER>
struct FastPair {
    // per-scenario constants
    float h, hh, h6, kv, kvz, inv_lr, lr_ratio, big;
    double b0, b1, dt;
    int n_rk4;

    __device__ __forceinline__ void init(const KP& P, double b0_, double b1_, double kv_) {
        h = (float)P.h; hh = (float)(P.h / 2); h6 = (float)(P.h / 6);
        kv = (float)kv_; inv_lr = (float)(1.0 / P.l_r); lr_ratio = (float)P.lr_ratio;
        kvz = fabsf(kv) < INFINITY ? kv : 0.0f;      // kv where the arc's share is 0 (arc_curv): kv itself unless it is non-finite
        big = 1.2676506e30f;      // 2^100
        b0 = b0_; b1 = b1_; dt = P.dt; n_rk4 = P.n_rk4;
    }
    static __device__ __forceinline__ void ssc(f2 d, f2& sd, f2& cd) {
        if (HI_ORDER) small_sincos2_hi(d, sd, cd); else small_sincos2(d, sd, cd);
    }
    // half-step (h/2-scaled) offsets
    static __device__ __forceinline__ void ssc_half(f2 d, f2& sd, f2& cd) {
        if (HI_ORDER) small_sincos2(d, sd, cd); else tiny_sincos2(d, sd, cd);
    }
    // K = kv [s >= b0] - kv [s >= b1] from the share d = [s >= b0] - [s >= b1] of the arc (0, 1, or a fraction within 2^-100 of a
    // break-point).  d kv as it stands would make 0 * kv = NaN of a non-finite kv BEFORE its arc, where pw_const (mpc.py:199)
    // and the whole-step variant say K = 0; with d = 0 the factor is kvz.  A finite kv has kvz = kv: the product's own bits.
    __device__ __forceinline__ f2 arc_curv(f2 d) const {
        f2 K;
#pragma unroll
        for (int q = 0; q < NV; ++q) K[q] = d[q] * (d[q] == 0.0f ? kvz : kv);
        return K;
    }
    // curvature of both candidates at break-point-relative arguments e + o*2^100
    __device__ __forceinline__ f2 curv(f2 e0, f2 e1, f2 o) const {
        // scalar v_fma_f32 ... clamp (the packed form cannot carry the clamp the compiler folds in)
        f2 c0, c1;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            c0[q] = __builtin_amdgcn_fmed3f(fmaf(o[q], big, e0[q]), 0.0f, 1.0f);
            c1[q] = __builtin_amdgcn_fmed3f(fmaf(o[q], big, e1[q]), 0.0f, 1.0f);
        }
        return arc_curv(c0 - c1);
    }

    // One RK4 sub-step, general curvature.  In/out: base pairs (s1,c1)=(sin,cos)(beta+epsi),
    // (s2,c2)=(sin,cos)(psi+beta); v1, ey, d0, d1 working values; acc_* increments of this control step.
    struct Work {
        f2 s1, c1, s2, c2, v1, ey, d0, d1, acc_s, acc_ey, acc_ep, acc_x, acc_y, acc_psi;
    };

    // Weighted stage sums in factorised form.  With per-stage offsets (sdA,cdA), (sdB,cdB), (sdC,cdC) of the
    // (beta+epsi) angle and per-stage gains g_j:
    //     sum_j w_j g_j cos(theta1 + d_j) = c1 A - s1 B,   sum_j w_j g_j sin(theta1 + d_j) = s1 A + c1 B,
    //     A = g1 + 2 g2 cdA + 2 g3 cdB + g4 cdC,           B = 2 g2 sdA + 2 g3 sdB + g4 sdC          (w = 1,2,2,1)
    // Both branches of substep() evaluate these through the same two helpers, so they agree bit for bit
    // whenever K == 0 (then g_j = v_j * 1 and the offsets coincide with the psi offsets).
    static __device__ __forceinline__ void stage_sums(f2 g1, f2 g2, f2 g3, f2 g4, f2 sdA, f2 cdA, f2 sdB, f2 cdB,
                                                      f2 sdC, f2 cdC, f2& A, f2& B) {
        const f2 t2 = splat(2.0f) * g2, t3 = splat(2.0f) * g3;
        A = fma2(g4, cdC, fma2(t3, cdB, fma2(t2, cdA, g1)));
        B = fma2(g4, sdC, fma2(t3, sdB, t2 * sdA));
    }

    // MODE 0: general (K decided per stage argument); 1: K == 0 at every stage argument of every lane; 2: every stage
    // argument of every lane lies strictly inside the arc, K == kv.  All three give identical bits where they apply.
    // XY = false (search units whose obstacles are out of every candidate's reach): the Cartesian rows are not integrated
    template <int MODE, bool XY = true>
    __device__ __forceinline__ void substep(f2 a, f2 ha, f2 sblr, Work& w) const {
        constexpr bool K0 = MODE == 1, KC = MODE == 2;
        const f2 H = splat(h), HH = splat(hh), H6 = splat(h6), BIG = splat(big), ONE = splat(1.0f), TWO = splat(2.0f);
        const f2 v1 = w.v1;
        const f2 v2 = v1 + ha;            // stages 2,3
        const f2 v4 = v2 + ha;            // stage 4
        const f2 s1 = w.s1, c1 = w.c1;
        const f2 w1 = v1 * sblr, w2 = v2 * sblr, w4 = v4 * sblr;
        // psi offsets h/2 w1 (stage 2), h/2 w2 (stages 3 AND 4, frenet.py:111)
        f2 sd2, cd2, sd3, cd3;
        ssc_half(HH * w1, sd2, cd2);
        ssc_half(HH * w2, sd3, cd3);
        // psi advances by h w2 per sub-step in closed form (w is linear in v: w1 + 4 w2 + w4 = 6 w2); epsi advances by the
        // same amount minus the curvature term  corr = h/6 (K1 ds1 + 2 K2 ds2 + 2 K3 ds3 + K4 ds4), which is exactly 0
        // on the K == 0 branch -- there both base pairs are rotated by (sin,cos)(h w2) and nothing else.
        f2 As, Bs, Ae, Be, ip, sdC, cdC, sdP, cdP, corr = splat(0.0f);
        if (K0) {
            // K == 0 at every stage argument of every lane: 1 - K ey = 1 and depsi = dpsi, so the
            // (beta+epsi) stage offsets are the psi offsets and the gains are the speeds.
            ssc(H * w2, sdP, cdP);
            sdC = sdP; cdC = cdP;
            stage_sums(v1, v2, v2, v4, sd2, cd2, sd3, cd3, sdC, cdC, Ae, Be);
            As = Ae; Bs = Be;
            ip = H * w2;
        } else {
            const f2 e0 = fma2(w.d0, BIG, ONE), e1 = fma2(w.d1, BIG, ONE);
            const f2 ey = w.ey;
            f2 sdA, cdA, sdB, cdB, sa, ca;
            // ---- stage 1
            f2 K = KC ? splat(kv) : arc_curv(clamp01(e0) - clamp01(e1));
            const f2 g1 = v1 * rcp2(fma2(-K, ey, ONE));
            const f2 ds1 = g1 * c1;
            const f2 de1 = v1 * s1;
            const f2 kd1 = ds1 * K;
            const f2 dp1 = w1 - kd1;
            // ---- stage 2: arguments base + h/2 k1
            ssc_half(HH * dp1, sdA, cdA);
            sa = s1; ca = c1; rotate2(sa, ca, sdA, cdA);
            if (!KC) K = curv(e0, e1, HH * ds1);
            const f2 g2 = v2 * rcp2(fma2(-K, fma2(HH, de1, ey), ONE));
            const f2 ds2 = g2 * ca;
            const f2 de2 = v2 * sa;
            const f2 kd2 = ds2 * K;
            const f2 dp2 = w2 - kd2;
            // ---- stage 3: base + h/2 k2
            ssc_half(HH * dp2, sdB, cdB);
            sa = s1; ca = c1; rotate2(sa, ca, sdB, cdB);
            if (!KC) K = curv(e0, e1, HH * ds2);
            const f2 g3 = v2 * rcp2(fma2(-K, fma2(HH, de2, ey), ONE));
            const f2 ds3 = g3 * ca;
            const f2 de3 = v2 * sa;
            const f2 kd3 = ds3 * K;
            const f2 dp3 = w2 - kd3;
            // ---- stage 4: base + h k3 (only its cosine is needed individually, for depsi)
            ssc(H * dp3, sdC, cdC);
            if (!KC) K = curv(e0, e1, H * ds3);
            const f2 g4 = v4 * rcp2(fma2(-K, fma2(H, de3, ey), ONE));
            const f2 ds4 = g4 * fma2(c1, cdC, -(s1 * sdC));
            const f2 kd4 = ds4 * K;
            stage_sums(g1, g2, g3, g4, sdA, cdA, sdB, cdB, sdC, cdC, As, Bs);
            stage_sums(v1, v2, v2, v4, sdA, cdA, sdB, cdB, sdC, cdC, Ae, Be);
            ssc(H * w2, sdP, cdP);
            corr = H6 * (kd1 + TWO * kd2 + TWO * kd3 + kd4);
            ip = H * w2 - corr;
        }
        // ---- Frenet increments (frenet.py:113-115)
        const f2 is = H6 * fma2(c1, As, -(s1 * Bs));
        const f2 ie = H6 * fma2(s1, Ae, c1 * Be);
        // ---- Cartesian rows collapse to one rotation of (A,B) as well (stage 4 shares stage 3's offset)
        if (XY) {
            const f2 v34 = fma2(TWO, v2, v4);
            const f2 tv2 = TWO * v2;
            const f2 Ac = fma2(v34, cd3, fma2(tv2, cd2, v1));
            const f2 Bc = fma2(v34, sd3, tv2 * sd2);
            w.acc_x = fma2(H6, fma2(w.c2, Ac, -(w.s2 * Bc)), w.acc_x);
            w.acc_y = fma2(H6, fma2(w.s2, Ac, w.c2 * Bc), w.acc_y);
        }
        w.acc_psi = fma2(H6, w1 + splat(4.0f) * w2 + w4, w.acc_psi);
        w.acc_s += is; w.acc_ey += ie; w.acc_ep += ip;
        w.d0 += is; w.d1 += is; w.ey += ie; w.v1 = v4;
        // ---- base pairs for the next sub-step: (psi+beta) advances by h w2, (beta+epsi) by ip = h w2 - corr.
        // K == 0: corr = 0 exactly and ip = h w2 - 0, so ssc(ip) IS (sdP, cdP) -- the branches stay bit-identical.
        if (XY) rotate2(w.s2, w.c2, sdP, cdP);
        if (K0) {
            rotate2(w.s1, w.c1, sdP, cdP);
        } else {
            f2 sd, cd;
            ssc(ip, sd, cd);
            rotate2(w.s1, w.c1, sd, cd);
        }
    }

    // n_rk4 sub-steps of one control step.  The K == 0 branch (or the K == kv one) is taken when it is provably
    // exact for every active lane of the wave: straight route, or every lane's stage arguments stay outside (inside)
    // the arc [b0, b1] by the travel bound |ds| <= 2 |v| (1/(1 - K ey) < 2 for any state near the road).
    // The lanes of a wave may belong to different scenarios (emit uses UNIFORM = false: general branch only).
    // the n_rk4 sub-steps of one variant; the reference's discretisation (4) is unrolled: no loop-carried register copies
    template <int MODE, bool XY>
    __device__ __forceinline__ void run(f2 a, f2 ha, f2 sblr, Work& w) const {
        if (n_rk4 == 4) {
            substep<MODE, XY>(a, ha, sblr, w); substep<MODE, XY>(a, ha, sblr, w); substep<MODE, XY>(a, ha, sblr, w); substep<MODE, XY>(a, ha, sblr, w);
        } else {
            for (int j = 0; j < n_rk4; ++j) substep<MODE, XY>(a, ha, sblr, w);
        }
    }

    template <bool UNIFORM, bool XY = true>
    __device__ __forceinline__ void substeps(f2 a, f2 sblr, Work& w) const {
        const f2 ha = splat(hh) * a;
        if (!UNIFORM) {
            run<0, XY>(a, ha, sblr, w);
            return;
        }
        if (kv == 0.0f) {                      // straight route: scalar condition, hoisted
            run<1, XY>(a, ha, sblr, w);
            return;
        }
        {   // the whole control step: |travel| <= 2 dt (|v| + dt |a|)
            const f2 m = splat(2.0f * (float)dt) * (__builtin_elementwise_abs(w.v1) + splat((float)dt) * __builtin_elementwise_abs(a));
            const f2 lo = w.d0 + m, hi = w.d1 - m, in0 = w.d0 - m, in1 = w.d1 + m;
            // inside the arc the travel bound's factor 2 holds while |K ey| < 1/2 at every stage (igt_fast64.h substeps)
            const f2 key = splat(fabsf(kv)) * (__builtin_elementwise_abs(w.ey) + splat(0.5f) * m);
            bool clear = true, inside = true;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                clear &= (lo[q] < 0.0f) | (hi[q] > 0.0f);
                inside &= (in0[q] > 0.0f) & (in1[q] < 0.0f) & (key[q] < 0.5f);
            }
            if (__all(clear)) {
                run<1, XY>(a, ha, sblr, w);
                return;
            }
            if (__all(inside)) {
                run<2, XY>(a, ha, sblr, w);
                return;
            }
        }
        for (int j = 0; j < n_rk4; ++j) {
            // travel bound of this sub-step: |o| <= h |ds| <= 2 h (|v| + |h a|)
            const f2 m = splat(2.0f * h) * (__builtin_elementwise_abs(w.v1) + splat(2.0f) * __builtin_elementwise_abs(ha));
            const f2 lo = w.d0 + m, hi = w.d1 - m, in0 = w.d0 - m, in1 = w.d1 + m;
            const f2 key = splat(fabsf(kv)) * (__builtin_elementwise_abs(w.ey) + splat(0.5f) * m);
            bool clear = true, inside = true;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                clear &= (lo[q] < 0.0f) | (hi[q] > 0.0f);
                inside &= (in0[q] > 0.0f) & (in1[q] < 0.0f) & (key[q] < 0.5f);
            }
            if (__all(clear)) substep<1, XY>(a, ha, sblr, w);
            else if (__all(inside)) substep<2, XY>(a, ha, sblr, w);
            else substep<0, XY>(a, ha, sblr, w);
        }
    }
};

// ---------------------------------------------------------------------------------------
// one pass over a PAIR of candidates of one scenario
// ---------------------------------------------------------------------------------------
// CAND = CAND_LATTICE / CAND_RAMP_HOLD: both candidates share the steering profile (c and c+64 have the same j)
// and satisfy the input box / rate limits by construction; CAND_TABLE: controls come from the table and are checked.
// O: the options of igt_roll_options.h that have a meaning here.  Without ROLL_BOOK (emit) cost and verdicts are skipped, only
// the trajectory is produced.  ROLL_LEAVE_CKPT (search, small batches): the state at N/4, N/2, 3N/4 is left in HBM for emit
// (in.ck).  ROLL_RESUME (emit): only control steps [in.seg.k0, in.seg.k1) are rolled, resuming from such a record.
// ROLL_NO_XY (search only, decided per unit by obstacles_out_of_reach; never with ROLL_LEAVE_CKPT): x, y are neither integrated
// nor judged.
template <int CAND, bool HI_ORDER, unsigned O, typename T, class Sink>
__device__ __forceinline__ void rollout_pair(const KP& P, const Scenario<T>& S, const int (&cidx)[NV],
                                             const double* __restrict__ table,
                                             const double* __restrict__ cinf, Sink& sink, double (&Jout)[NV],
                                             unsigned (&vout)[NV], double (&sN)[NV], double (&vN)[NV], const PairIn& in = PairIn()) {
    static_assert(roll_supported(O) && !(O & (ROLL_STEER_TABLE | ROLL_STEP_TABLE | ROLL_EY_FOLDED | ROLL_PART_D)), "float64 only");
    constexpr bool BOOK = (O & ROLL_BOOK) != 0, UNIFORM = (O & ROLL_UNIFORM) != 0, EARLY_EXIT = (O & ROLL_EARLY_EXIT) != 0;
    constexpr bool CKPT = (O & ROLL_LEAVE_CKPT) != 0, SEG = (O & ROLL_RESUME) != 0, XY = !(O & ROLL_NO_XY);
    const Ckpt& ck = in.ck;
    const Seg& seg = in.seg;
    const unsigned long long* inc = in.inc;
    constexpr bool KEEP_PSI = Sink::kKeepsStates || CKPT || SEG;
    // inc (search, tracking family, progress cost; may be null): the scenario's incumbent key -- a candidate whose lower bound
    // LB_k = J_k - (s_k - s_0) - rem_k exceeds it cannot win (igt_fast64.h rollout_one has the derivation; here the stage terms
    // are float sums, so the margin of the comparison is 1e-4 instead of 1e-9)
    constexpr bool BOUND = roll_bound(CAND, O);
    constexpr bool LATTICE = CAND == CAND_LATTICE || CAND == CAND_RAMP_HOLD;   // generated, steering shared by the pair
    constexpr bool GENERATED = CAND != CAND_TABLE;                           // box / rate limits hold by construction
    // search only needs feasible-or-not: the float-side verdicts (|ey|, box v, collision) are folded into one running
    // maximum per candidate, compared with the tolerance when it is read (x > tol for some x  <=>  max x > tol; a NaN
    // operand is ignored by both forms).  Everything that reports verdict BITS keeps them.
    constexpr bool LEAN = roll_lean(O);
    float gmax[NV];
    typedef FastPair<HI_ORDER> FP;
    FP fp;
    fp.init(P, S.b0, S.b1, S.kv);
    double s[NV], ey[NV], ep[NV], v[NV], x[NV], y[NV], psi[NV], J[NV], a_d[NV], df_d[NV], da[NV], ddf = 0.0, ddq[NV];
    unsigned viol[NV];
    bool dead = false;     // EARLY_EXIT: the whole slice is already infeasible
    const float ey_lim = (float)P.ey_lim, tol = (float)P.tol, vmin = (float)P.v_min, vmax = (float)P.v_max;
    const float w_u = (float)P.w_u, dmin2 = (float)P.dmin2, ratio2 = fp.lr_ratio * fp.lr_ratio;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        x[q] = S.x0[0]; y[q] = S.x0[1]; s[q] = S.x0[2]; ey[q] = S.x0[3]; ep[q] = S.x0[4]; v[q] = S.x0[5]; psi[q] = S.x0[6];
        a_d[q] = S.a_prev; df_d[q] = S.df_prev;
        if (CAND == CAND_LATTICE) {
            // da_i = -ra + (2 ra) i/(G-1), ddf_j likewise (SURVEY 8d; oracle candidates_lattice)
            const int i = cidx[q] / P.G, j = cidx[q] - i * P.G;
            da[q] = -P.rate_a + (2 * P.rate_a) * (double)i / (double)(P.G - 1);
            if (q == 0) ddf = -P.rate_df + (2 * P.rate_df) * (double)j / (double)(P.G - 1);
        } else if (CAND == CAND_RAMP_HOLD) {
            // da / ddf hold the OFFSETS of the targets from the base sequence here (igt_device.h cand_m, ramp_base)
            const int i = cidx[q] / P.G, j = cidx[q] - i * P.G;
            da[q] = S.cpar[0] + cand_m(i, P.G, P.refine_it == 0) * S.cpar[2];
            if (q == 0) ddf = S.cpar[1] + cand_m(j, P.G, P.refine_it == 0) * S.cpar[3];
        } else if (CAND == CAND_TRACK) {
            // acceleration as ramp-hold; ddq = slip-angle offset of the steering feedback (igt_device.h track_steer)
            const int i = cidx[q] / P.G, j = cidx[q] - i * P.G;
            da[q] = S.cpar[0] + cand_m(i, P.G, P.refine_it == 0) * S.cpar[2];
            ddq[q] = S.cpar[1] + cand_m(j, P.G, P.refine_it == 0) * S.cpar[3];
        }
        if (CAND != CAND_TRACK) ddq[q] = 0.0;
        J[q] = 0.0; viol[q] = 0; gmax[q] = -3.0e38f;
        if (!SEG || seg.k0 == 0) sink.state(q, 0, S.x0);
    }
    // (sin,cos)(psi_0): the same for every candidate of the scenario
    float sp0, cp0;
    sincos_reduced(S.x0[6], sp0, cp0);
    typename FP::Work w;
    w.d0 = w.d1 = splat(0.0f);
    w.s2 = splat(sp0); w.c2 = splat(cp0);      // carried as (sin,cos)(psi + beta_k); beta_{-1} = 0
    f2 cb_prev = splat(1.0f), sb_prev = splat(0.0f);
    float ox_next = 0.0f, oy_next = 0.0f;      // obstacle 0 at the state the next trip books
    if (SEG && seg.load) {                     // resume at k0 from the checkpoint record
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const double* r = seg.load + seg.slot0 + 64 * q;
            x[q] = r[0 * SEG_SLOTS]; y[q] = r[1 * SEG_SLOTS]; s[q] = r[2 * SEG_SLOTS]; ey[q] = r[3 * SEG_SLOTS];
            ep[q] = r[4 * SEG_SLOTS]; v[q] = r[5 * SEG_SLOTS]; psi[q] = r[6 * SEG_SLOTS]; J[q] = r[7 * SEG_SLOTS];
            a_d[q] = r[8 * SEG_SLOTS]; df_d[q] = r[9 * SEG_SLOTS];
            const float2 sc = *reinterpret_cast<const float2*>(r + 10 * SEG_SLOTS);
            const float2 bp = *reinterpret_cast<const float2*>(r + 11 * SEG_SLOTS);
            w.s2[q] = sc.x; w.c2[q] = sc.y; cb_prev[q] = bp.x; sb_prev[q] = bp.y;
        }
    }
    const int k_begin = SEG ? seg.k0 : 0, k_end = SEG ? seg.k1 : P.N;
    double rem[NV], jcut = (double)INFINITY, seg_scale = 0.0;
#pragma unroll
    for (int q = 0; q < NV; ++q) rem[q] = 0.0;
    if (BOUND && inc) {
        seg_scale = progress_slack<T>(P, S) * P.dt;
        if (seg_scale > 0.0) {          // the rows' own (a, v) recurrences rolled ahead: the statements of the loop below
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                double a2 = S.a_prev, v2 = S.x0[5];
                for (int k = 0; k < P.N; ++k) {
                    double ba, bdf;
                    ramp_base<T>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
                    // Without the speed cap where the speed box keeps feasible speeds from going negative (v_min >= 0): the target map
                    // is monotone in (a_{k-1}, target), so the uncapped accelerations -- and speeds -- lie above the capped ones, and
                    // a sum over them still bounds what the row can gain (the cap only ever acts near v_max > 0).  The capped
                    // recurrence costs a square root and a quotient per step, twice per lane here, ahead of every unit; the float64
                    // path reads the sums accel_rows_kernel leaves instead.
                    // The uncapped |v| is not an upper bound everywhere though: a feasible row's capped v_k, k < N, is only >= -tol,
                    // and v_N is not box-checked (v_N >= v_N-1 + dt a_min >= -tol - |a_min| dt).  So |v_k capped| <= |v_k uncapped| + tol
                    // for k < N and + |a_min| dt more at k = N: those margins are added to the steps' terms below.
                    if (P.v_min >= 0.0) {
                        const double ta = track_accel_target_uncapped(P, k, ba, da[q]);
                        a2 = clampd(a2 + clampd(ta - a2, -P.rate_a, P.rate_a), P.a_min, P.a_max);
                    } else {
                        a2 = track_accel_next(P, k, ba, da[q], v2, a2);
                    }
                    const double vn = fma(fp.dt, a2, v2);
                    rem[q] += fmax(fabs(v2), fabs(vn));
                    v2 = vn;
                }
                if (P.v_min >= 0.0) rem[q] += fma((double)P.N, P.tol, fabs(P.a_min) * P.dt);
                rem[q] *= seg_scale * (1.0 + 1e-6);
            }
        } else {
            inc = nullptr;
        }
    }

    for (int k = k_begin; k < k_end; ++k) {
        if (CKPT && ck.base && k > 0 && k % ck.every == 0) {      // state at k = part boundary -> record (k / every - 1)
            double* rec = ck.base + ((size_t)(k / ck.every - 1) * ck.n_units + ck.unit) * SEG_UNIT_DOUBLES;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                if (viol[q] != 0 || (LEAN && gmax[q] > tol)) continue;      // emit only ever asks for a feasible winner
                double* r = rec + ck.slot0 + 64 * q;
                r[0 * SEG_SLOTS] = x[q]; r[1 * SEG_SLOTS] = y[q]; r[2 * SEG_SLOTS] = s[q]; r[3 * SEG_SLOTS] = ey[q];
                r[4 * SEG_SLOTS] = ep[q]; r[5 * SEG_SLOTS] = v[q]; r[6 * SEG_SLOTS] = psi[q]; r[7 * SEG_SLOTS] = J[q];
                r[8 * SEG_SLOTS] = a_d[q]; r[9 * SEG_SLOTS] = df_d[q];
                *reinterpret_cast<float2*>(r + 10 * SEG_SLOTS) = make_float2(w.s2[q], w.c2[q]);
                *reinterpret_cast<float2*>(r + 11 * SEG_SLOTS) = make_float2(cb_prev[q], sb_prev[q]);
            }
        }
        // ---- controls of step k (double)
        f2 a, cb, sb, tu;
        if (CAND == CAND_LATTICE) {
            df_d[0] = clampd(df_d[0] + ddf, -P.df_max, P.df_max);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                df_d[q] = df_d[0];
                a_d[q] = clampd(a_d[q] + da[q], P.a_min, P.a_max);
            }
        } else if (CAND == CAND_RAMP_HOLD) {
            double ba, bdf;
            ramp_base<T>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
            const double tdf = clampd(bdf + ddf, -P.df_max, P.df_max);
            df_d[0] = clampd(df_d[0] + clampd(tdf - df_d[0], -P.rate_df, P.rate_df), -P.df_max, P.df_max);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                df_d[q] = df_d[0];
                const double ta = clampd(ba + da[q], P.a_min, P.a_max);
                a_d[q] = clampd(a_d[q] + clampd(ta - a_d[q], -P.rate_a, P.rate_a), P.a_min, P.a_max);
            }
        } else if (CAND == CAND_TRACK) {
            double ba, bdf;
            ramp_base<T>(S.ws, P.N, k, S.a_prev, S.df_prev, ba, bdf);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                a_d[q] = track_accel_next(P, k, ba, da[q], (double)v[q], a_d[q]);
                df_d[q] = track_steer(P, df_d[q], ey[q], ep[q], ddq[q]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const double an = table[((size_t)cidx[q] * 2 + 0) * P.N + k];
                const double dn = table[((size_t)cidx[q] * 2 + 1) * P.N + k];
                // input-rate (mpc.py:301-312, u_{-1} = u_prev) and input box (mpc.py:318-321)
                if (BOOK) {
                    if (fmax(fabs(an - a_d[q]) - P.rate_a, fabs(dn - df_d[q]) - P.rate_df) > P.tol) viol[q] |= VIOL_RATE;
                    if (fmax(fmax(P.a_min - an, an - P.a_max), fmax(-P.df_max - dn, dn - P.df_max)) > P.tol)
                        viol[q] |= VIOL_BOX_U;
                }
                a_d[q] = an; df_d[q] = dn;
            }
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            sink.ctrl(q, k, a_d[q], df_d[q]);
            a[q] = (float)a_d[q];
            if (!LATTICE || q == 0) {
                // beta = atan(r tan df), r = l_r/(l_f+l_r):  cos(beta) = c/n, sin(beta) = r s/n,
                // n = sqrt(c^2 + r^2 s^2), (s,c) = (sin,cos)(df)   (|df| < pi/2)
                float sdf, cdf;
                if (GENERATED && P.df_small) sincos_quadrant0((float)df_d[q], sdf, cdf);   // |df| <= df_max < pi/4
                else sincos_reduced(df_d[q], sdf, cdf);
                const float n = __builtin_amdgcn_rsqf(fmaf(ratio2 * sdf, sdf, cdf * cdf));   // argument in [r^2, 1]
                cb[q] = cdf * n;
                sb[q] = fp.lr_ratio * sdf * n;
                const float dff = (float)df_d[q];
                tu[q] = dff * dff;
            } else {
                cb[q] = cb[0]; sb[q] = sb[0]; tu[q] = tu[0];
            }
        }
        const f2 sblr = sb * splat(fp.inv_lr);
        tu = splat(w_u) * fma2(a, a, tu);                              // mpc.py:362
        // ---- bookkeeping of state k + float working set of this control step
        float epf[NV];
        bool quadrant0 = true;       // every heading error of the lane within (-pi/4, pi/4)
#pragma unroll
        for (int q = 0; q < NV; ++q) { epf[q] = (float)ep[q]; quadrant0 &= fabsf(epf[q]) < QUADRANT0; }
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            w.ey[q] = (float)ey[q];
            w.v1[q] = (float)v[q];
            if (BOOK) {
                const float t = fmaf(w.ey[q], w.ey[q], fmaf(epf[q], epf[q], tu[q]));    // mpc.py:362-364
                J[q] += (double)t;
                if (LEAN) {
                    gmax[q] = fmaxf(gmax[q], fabsf(w.ey[q]) - ey_lim);                               // mpc.py:296-299
                    gmax[q] = fmaxf(gmax[q], fmaxf(vmin - w.v1[q], w.v1[q] - vmax));                 // mpc.py:316-317 (k < N)
                } else {
                    if (fabsf(w.ey[q]) - ey_lim > tol) viol[q] |= VIOL_EY;          // mpc.py:296-299
                    if (fmaxf(vmin - w.v1[q], w.v1[q] - vmax) > tol) viol[q] |= VIOL_BOX_V;   // mpc.py:316-317 (k < N)
                }
            }
            if (fp.kv != 0.0f) {               // break-point-relative arc length (unused on straight routes)
                w.d0[q] = (float)(s[q] - fp.b0);
                w.d1[q] = (float)(s[q] - fp.b1);
            }
        }
        if (BOOK && k == P.N - 1) {                                    // mpc.py:177-180
#if IGT_NV == 2
            terminal_viol2(P, v, a_d, cinf, viol);
#else
            viol[0] |= terminal_viol(P, v[0], a_d[0], cinf);
#endif
        }
        // (sin,cos)(epsi): heading errors beyond pi/4 are rare, so the range reduction is skipped when no lane needs it
        if (__all(quadrant0)) {
#pragma unroll
            for (int q = 0; q < NV; ++q) { float se, ce; sincos_quadrant0(epf[q], se, ce); w.s1[q] = se; w.c1[q] = ce; }
        } else {
#pragma unroll
            for (int q = 0; q < NV; ++q) { float se, ce; sincos_reduced(ep[q], se, ce); w.s1[q] = se; w.c1[q] = ce; }
        }
        if (BOUND && inc) {
            if ((k & 3) == 0) {      // re-read every fourth step (agent scope: the scenario's units may run on different XCDs)
                const double ji = cost_of_key(__hip_atomic_load(inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                jcut = ji + 1e-4 * (1.0 + fabs(ji));
            }
#pragma unroll
            for (int q = 0; q < NV; ++q)
                if ((J[q] - (s[q] - S.x0[2])) - rem[q] > jcut) viol[q] |= VIOL_PRUNED;
        }
        if (BOOK && UNIFORM && EARLY_EXIT) {
            // search only: once every candidate of the slice has failed a verdict, nothing rolled further can win
            bool lost = true;
#pragma unroll
            for (int q = 0; q < NV; ++q) lost &= (viol[q] != 0) | (LEAN && gmax[q] > tol);
            if (__all(lost) && !(P.dev & DEV_NO_EARLY_EXIT)) { dead = true; break; }
        }
        if (BOOK && XY) {                                              // collision, mpc.py:223-226 (k >= 1)
            // obstacle 0 of the NEXT state is requested now and used one trip later: a scalar load's latency is
            // longer than the bookkeeping between here and the sub-steps, and few waves share a SIMD
            const float ox0 = ox_next, oy0 = oy_next;
            if (P.n_obs > 0) { ox_next = S.obs[k + 1]; oy_next = S.obs[(P.N + 1) + k + 1]; }
            for (int o = 0; o < P.n_obs && k >= 1; ++o) {
                const double ox = o == 0 ? (double)ox0 : (double)S.obs[(o * 2 + 0) * (P.N + 1) + k];
                const double oy = o == 0 ? (double)oy0 : (double)S.obs[(o * 2 + 1) * (P.N + 1) + k];
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const float dx = (float)(x[q] - ox), dy = (float)(y[q] - oy);
                    if (LEAN) gmax[q] = fmaxf(gmax[q], dmin2 - fmaf(dx, dx, dy * dy));
                    else if (dmin2 - fmaf(dx, dx, dy * dy) > tol) viol[q] |= VIOL_COLLISION;
                }
            }
        }
        rotate2(w.s1, w.c1, sb, cb);                                   // (sin,cos)(beta + epsi)
        // (sin,cos)(psi + beta_k) from (psi + beta_{k-1}): rotate by beta_k - beta_{k-1}, re-normalise
        {
            const f2 sdb = fma2(sb, cb_prev, -(cb * sb_prev));
            const f2 cdb = fma2(cb, cb_prev, sb * sb_prev);
            if (XY) {
                rotate2(w.s2, w.c2, sdb, cdb);
                const f2 n = fma2(w.s2, w.s2, w.c2 * w.c2);
                const f2 r = fma2(n, splat(-0.5f), splat(1.5f));
                w.s2 *= r; w.c2 *= r;
            }
            cb_prev = cb; sb_prev = sb;
        }
        w.acc_s = splat(0.f); w.acc_ey = splat(0.f); w.acc_ep = splat(0.f);
        w.acc_x = splat(0.f); w.acc_y = splat(0.f); w.acc_psi = splat(0.f);
        fp.template substeps<UNIFORM, XY>(a, sblr, w);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            s[q] += (double)w.acc_s[q]; ey[q] += (double)w.acc_ey[q]; ep[q] += (double)w.acc_ep[q];
            if (XY) { x[q] += (double)w.acc_x[q]; y[q] += (double)w.acc_y[q]; }
            if (KEEP_PSI) psi[q] += (double)w.acc_psi[q];      // psi feeds nothing back (search without checkpoints: dead)
            if (BOUND && inc) rem[q] -= seg_scale * fmax(fabs(v[q]), fabs(fma(fp.dt, a_d[q], v[q])));
            v[q] = fma(fp.dt, a_d[q], v[q]);
            const double nxt[7] = {x[q], y[q], s[q], ey[q], ep[q], v[q], psi[q]};
            sink.state(q, k + 1, nxt);
        }
    }
    if (dead) {            // costs are meaningless; the verdict bits that ended the roll are what is reported
#pragma unroll
        for (int q = 0; q < NV; ++q) { Jout[q] = 0.0; vout[q] = viol[q] | ((LEAN && gmax[q] > tol) ? VIOL_EY : 0u); sN[q] = 0.0; vN[q] = 0.0; }
        return;
    }
#pragma unroll
    for (int q = 0; q < NV && BOOK; ++q) {
        const float epf = (float)ep[q], eyq = (float)ey[q];
        J[q] += (double)fmaf(eyq, eyq, epf * epf);
        if (LEAN) gmax[q] = fmaxf(gmax[q], fabsf(eyq) - ey_lim);
        else if (fabsf(eyq) - ey_lim > tol) viol[q] |= VIOL_EY;
        for (int o = 0; XY && o < P.n_obs; ++o) {
            const float dx = (float)(x[q] - (o == 0 ? (double)ox_next : (double)S.obs[(o * 2 + 0) * (P.N + 1) + P.N]));
            const float dy = (float)(y[q] - (o == 0 ? (double)oy_next : (double)S.obs[(o * 2 + 1) * (P.N + 1) + P.N]));
            if (LEAN) gmax[q] = fmaxf(gmax[q], dmin2 - fmaf(dx, dx, dy * dy));
            else if (dmin2 - fmaf(dx, dx, dy * dy) > tol) viol[q] |= VIOL_COLLISION;
        }
        if (LEAN && gmax[q] > tol) viol[q] |= VIOL_EY;     // lean form: "some float-side verdict failed"
        if (!(fabs(x[q]) < 1e300 && fabs(y[q]) < 1e300 && fabs(s[q]) < 1e300 && fabs(ey[q]) < 1e300 &&
              fabs(ep[q]) < 1e300 && fabs(psi[q]) < 1e300))
            viol[q] |= VIOL_NONFINITE;
        sN[q] = s[q]; vN[q] = v[q];
        Jout[q] = J[q]; vout[q] = viol[q];
    }
    if (!BOOK) {
#pragma unroll
        for (int q = 0; q < NV; ++q) { Jout[q] = 0.0; vout[q] = 0; sN[q] = 0.0; vN[q] = 0.0; }
    }
}

