// igt_kernels_f64.hip -- gfx950 kernels of the float64 entry points (the reference's precision) and their launchers:
//   search_f64_kernel_*   persistent waves, one unit -- 64 candidates of one scenario -- at a time (igt_fast64.h); _cap: small
//                         batches, every unit also keeps its 64 trajectories
//   search_cand_*_f64_kernel   per-scenario candidate sets U[B,C,2,N]: one wave per unit, the unit's slab staged in LDS, or
//                         search_unit64 on the scenario's own table
//   accel_rows_kernel     ahead of the search (batches above 1024 scenarios): the acceleration rows that can still win
//   emit_f64_kernel       one lane per scenario: the winner re-rolled with the same arithmetic -> x*[7,N+1], u*[2,N]
//   emit_gather_f64_kernel   small batches: the winner's trajectory copied out of the unit that rolled it
//   rollout_all_f64_kernel   debug / parity: every candidate's trajectory, cost and verdict bits
//   polish_f64_kernel     projected-gradient steps on the winner (forward-difference or adjoint gradient; Newton direction)
//   value_trials_f64_kernel / value_accept_f64_kernel   the same under the value-network cost, around the network's kernels
//   cost_gradient_f64_kernel   dJ/du of the progress cost for one control sequence per scenario (igt_adjoint64.h); templated on the
//                         terminal term: the two sweeps of igt_cost_gradient_vn_f64 around the value network are instantiations
//   search_kernel / emit_kernel / rollout_all_kernel<ExactStepper<double>>   the oracle's operation order (IGT_DEV_FLAGS=1024)
//   search_literal_f64_kernel   the literal north_star mapping, a measurement variant (IGT_DEV_FLAGS=2048)
// Compiled on its own so that the two heavy translation units build in parallel.
#include "igt_device.h"
#include "igt_fast64.h"
#include "igt_adjoint64.h"
#include "igt_launch.h"
#include "igt_kernels_common.h"

namespace igt {

#if IGT_DEV_KERNELS   // the oracle-order kernels (IGT_DEV_FLAGS = 1024)
template <class Stepper, typename T, int NC, bool SHARED_DF, bool VALUE>
__global__ __launch_bounds__(256) void search_kernel(KP P, int B, const T* __restrict__ x0,
                                                     const T* __restrict__ u_prev,
                                                     const T* __restrict__ kparams,
                                                     const uint32_t* __restrict__ flags,
                                                     const T* __restrict__ obs,
                                                     const double* __restrict__ table,
                                                     const double* __restrict__ cinf, Centre<T> cpar,
                                                     T* __restrict__ cost_out, int32_t* __restrict__ argmin_out,
                                                     int32_t* __restrict__ status_out, T* __restrict__ rec_sN,
                                                     T* __restrict__ rec_vN, double* __restrict__ rec_J,
                                                     uint32_t* __restrict__ rec_viol) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    Scenario<T> S;
    load_scenario<T>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);

    double bestJ = 0.0;
    int bestC = -1;
    NullSink sink;
    const int passes = P.C / (64 * NC);
    for (int p = 0; p < passes; ++p) {
        int cidx[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) cidx[q] = (p * NC + q) * 64 + lane;
        double J[NC], sN[NC], vN[NC];
        unsigned viol[NC];
        rollout_pass<Stepper, NC, SHARED_DF, T>(P, S, cidx, table, cinf, sink, J, viol, sN, vN);
        if (VALUE) {   // terminal value network: leave the terminal term to value_kernel (mpc.py:369)
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const size_t idx = (size_t)b * P.C + cidx[q];
                rec_sN[idx] = (T)sN[q]; rec_vN[idx] = (T)vN[q]; rec_J[idx] = J[q]; rec_viol[idx] = viol[q];
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const double Jq = J[q] - (sN[q] - S.x0[2]);  // mpc.py:372
            const bool ok = (viol[q] == 0) && finite_d(Jq);
            // candidates arrive in increasing index per lane: strict '<' keeps the lowest index
            if (ok && (bestC < 0 || Jq < bestJ)) { bestJ = Jq; bestC = cidx[q]; }
        }
    }
    // wave butterfly arg-min, ties -> lowest candidate index: wave_argmin (igt_device.h) written out, it must agree with it
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double oJ = __shfl_xor(bestJ, off, 64);
        const int oC = __shfl_xor(bestC, off, 64);
        const bool take = (oC >= 0) && (bestC < 0 || oJ < bestJ || (oJ == bestJ && oC < bestC));
        if (take) { bestJ = oJ; bestC = oC; }
    }
    if (VALUE) return;
    if (lane == 0) write_verdict<T>(b, bestJ, bestC, cost_out, argmin_out, status_out);
}

template <class Stepper, typename T>
__global__ __launch_bounds__(64) void emit_kernel(KP P, int B, const T* __restrict__ x0,
                                                  const T* __restrict__ u_prev, const T* __restrict__ kparams,
                                                  const uint32_t* __restrict__ flags, const T* __restrict__ obs,
                                                  const double* __restrict__ table,
                                                  const double* __restrict__ cinf, Centre<T> cpar,
                                                  const int32_t* __restrict__ argmin, T* __restrict__ x_out,
                                                  T* __restrict__ u_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    T* xo = x_out + (size_t)b * 7 * (P.N + 1);
    T* uo = u_out + (size_t)b * 2 * P.N;
    const int c = argmin[b];
    if (c < 0) { no_trajectory<T>(P, xo, uo); return; }
    Scenario<T> S;
    load_scenario<T>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
    StoreSink<T> sink{xo, uo, P.N};
    const int cidx[1] = {c};
    double J[1], sN[1], vN[1];
    unsigned viol[1];
    rollout_pass<Stepper, 1, false, T>(P, S, cidx, table, cinf, sink, J, viol, sN, vN);
}

template <class Stepper, typename T>
__global__ __launch_bounds__(256) void rollout_all_kernel(KP P, int B, const T* __restrict__ x0,
                                                          const T* __restrict__ u_prev,
                                                          const T* __restrict__ kparams,
                                                          const uint32_t* __restrict__ flags,
                                                          const T* __restrict__ obs,
                                                          const double* __restrict__ table,
                                                          const double* __restrict__ cinf, Centre<T> cpar, T* __restrict__ X_all,
                                                          T* __restrict__ U_all, T* __restrict__ cost_all,
                                                          uint32_t* __restrict__ viol_all, T* __restrict__ rec_sN,
                                                          T* __restrict__ rec_vN, double* __restrict__ rec_J,
                                                          uint32_t* __restrict__ rec_viol) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    Scenario<T> S;
    load_scenario<T>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
    for (int c = lane; c < P.C; c += 64) {
        const size_t bc = (size_t)b * P.C + c;
        StoreSink<T> sink{X_all ? X_all + bc * 7 * (P.N + 1) : nullptr, U_all ? U_all + bc * 2 * P.N : nullptr, P.N};
        const int cidx[1] = {c};
        double J[1], sN[1], vN[1];
        unsigned viol[1];
        rollout_pass<Stepper, 1, false, T>(P, S, cidx, table, cinf, sink, J, viol, sN, vN);
        if (rec_J) {   // value-net cost: value_kernel adds the terminal term and fills cost_all / viol_all
            rec_sN[bc] = (T)sN[0]; rec_vN[bc] = (T)vN[0]; rec_J[bc] = J[0]; rec_viol[bc] = viol[0];
            continue;
        }
        const double Jq = J[0] - (sN[0] - S.x0[2]);
        if (!finite_d(Jq)) viol[0] |= VIOL_NONFINITE;
        cost_all[bc] = (T)Jq;
        viol_all[bc] = viol[0];
    }
}


#endif  // IGT_DEV_KERNELS

// ---------------------------------------------------------------------------------------
// float64 path (igt_fast64.h): one candidate per lane, W = C/64 units per scenario
// ---------------------------------------------------------------------------------------
// Generated G x G families with W * 64 == C and W | G: unit p takes G/W STEERING values (all G accelerations), handed out
// from the centre of the range outwards, as the float path does with its 128-candidate slices -- the extreme-steering
// units fail as a whole within a few steps and leave through the early exit.  Otherwise: chunks of 64 in index order
// (igt_kernels_common.h unit_layout / unit_candidate).
// The tracking family's steering is a feedback on the rolled state: its candidates hardly ever fail on |e_y|, they fail on
// what the ACCELERATION profile decides (collision, speed box, terminal set), so its units are cut along the acceleration
// axis instead -- unit p takes G/W consecutive acceleration offsets with all G steering offsets (tools/death_steps_track.py:
// 90.8 % of the wave-steps executed against 94.1 % with steering slices).
//
// Acceleration rows that cannot win.  In the generated families the acceleration sequence of candidate (i, j) depends on the
// row i alone, the speed is v_{k+1} = v_k + dt a_k, and two of the verdicts -- the speed box (mpc.py:316-317) and the terminal
// set on (v_{N-1}, a_{N-1}) (mpc.py:177-180) -- read nothing else: a row that fails one of them is infeasible in all of its
// G columns whatever the steering does.  accel_rows_kernel rolls the G scalar recurrences of a scenario ahead of the search
// (the same expressions as rollout_one, so the same bits) and leaves the rows that survive as a bit mask; the units are then
// made of live rows only:
//   * steering slices (lattice, ramp-hold): the scenario's G R live candidates are numbered column by column from the centre
//     of the steering range outwards and unit p takes numbers 64 p .. 64 p + 63 -- ceil(G R / 64) units instead of W, a column
//     may straddle two of them (benchmark batch: 10.7 of 16 rows live, 3.1 units instead of 4, 77 % of the wave-steps).  Where
//     the unit's steering table would not hold the floor(63 / R) + 2 columns such a unit can touch -- or with
//     IGT_DEV_FLAGS = 4194304 -- a unit holds floor(64 / R) whole columns instead (3.5 units, 83 %);
//   * acceleration-axis units (tracking): unit p takes the live rows of rank p G/W .. (p+1) G/W - 1: ceil(R W / G) units.
// Slices beyond that are empty (the wave moves on), lanes without a candidate idle with "lost" set from the start.
// A mask of all ones is the layout without this (IGT_DEV_FLAGS = 2097152; small batches, packs_live_rows).
//
// one lane per (scenario, acceleration row), 64 / G scenarios per wave: the row's (a_k, v_k) recurrence with the two verdicts that
// read nothing else -- the statements of rollout_one (igt_fast64.h), in its order; what load_scenario reads of the scenario for
// them (a_prev, v_0, the warm start, the refinement centre) is read per lane here
//
// QUEUES (batches whose search queues are sorted, B <= 4096 at 256 candidates): the first eight workgroups of the same launch
// sort one queue each (build_queue, eight trips of 256 threads) while the others roll the rows -- one launch instead of two
// (the queue builder's own launch cost 7 us of a 236 us solve).  The two kinds of workgroup do not talk to each other: the
// queues are sorted without the masks, so a slice beyond a scenario's live rows' units is sorted like any other slice of
// its class and the search wave that takes it finds it empty and moves on.  (Sorting them last needs the masks first: as
// a second launch that is the 7 us; inside this one it was built with tickets and a device-scope fence per workgroup and
// cost 20 us, profiles/r04_ab_fused_prelude.txt.)
//
// THREADS: the workgroup.  ROWS_THREADS_WIDE (four waves; the queue builders take up to eight trips of 256 threads), or -- where
// solves overlap, igt_launch.h plan_search64 rows_threads -- ROWS_THREADS_NARROW: one wave, which starts wherever a single wave
// slot is free beside the resident searches (the builders then take up to 32 trips of 64 threads: the same stable sort, the
// same order table).  The lane mapping is the same either way.
template <int CAND, bool QUEUES, int THREADS>
__global__ __launch_bounds__(THREADS) void accel_rows_kernel(KP P, int B, const double* __restrict__ x0,
                                                         const double* __restrict__ u_prev, const uint32_t* __restrict__ flags,
                                                         const double* __restrict__ cinf, Centre<double> cpar,
                                                         unsigned long long* __restrict__ row_mask, double* __restrict__ row_rem,
                                                         int W, const double* __restrict__ kparams, unsigned* __restrict__ order,
                                                         int order_stride, unsigned* __restrict__ work_counter, int pool_units) {
    if constexpr (QUEUES) {
        if (blockIdx.x < 8) {      // pool_units > 0: one item per scenario (search_pool64)
            build_queue<double, THREADS, QB_THREADS * QB_TRIPS / THREADS>(P, B, pool_units > 0 ? 1 : W, (int)blockIdx.x, x0, kparams,
                                                                         order, order_stride, work_counter, nullptr, true, pool_units);
            return;
        }
    }
    const int lane = threadIdx.x & 63, lg = __ffs(P.G) - 1;                  // G is a power of two (igt_api.hip)
    const int per_wave = 64 >> lg;                                           // scenarios per wave
    const int wave = ((int)blockIdx.x - (QUEUES ? 8 : 0)) * (THREADS / 64) + (int)(threadIdx.x >> 6);
    const int b = wave * per_wave + (lane >> lg), i = lane & (P.G - 1);
    bool live = false;
    if (b < B) {
        const double a_prev = u_prev[(size_t)b * 2 + 0], df_prev = u_prev[(size_t)b * 2 + 1];
        const double* ws = (cpar.ws && (flags[b] & 2u)) ? cpar.ws + (size_t)b * 2 * P.N : nullptr;      // load_scenario's S.ws
        double c0 = 0.0, c2 = P.N * P.rate_a;                                                           // ... and S.cpar[0], [2]
        if (cpar.cpar) { c0 = cpar.cpar[(size_t)b * 4 + 0]; c2 = cpar.cpar[(size_t)b * 4 + 2]; }
        double da;
        if (CAND == CAND_LATTICE) da = -P.rate_a + (2 * P.rate_a) * (double)i / (double)(P.G - 1);
        else da = c0 + cand_m(i, P.G, P.refine_it == 0) * c2;
        double a = a_prev, v = x0[(size_t)b * 7 + 5], g = -1.0e300, travel = 0.0;
        unsigned viol = 0;
        bool twin = CAND == CAND_TRACK && i > 0;          // so far the row's accelerations are those of the row below it
        for (int k = 0; k < P.N; ++k) {
            if (CAND == CAND_LATTICE) {
                a = clampd(a + da, P.a_min, P.a_max);
            } else {
                double ba, bdf;
                ramp_base<double>(ws, P.N, k, a_prev, df_prev, ba, bdf);
                if (CAND == CAND_TRACK) {
                    a = track_accel_next(P, k, ba, da, v, a);
                } else {
                    const double ta = clampd(ba + da, P.a_min, P.a_max);
                    a = clampd(a + clampd(ta - a, -P.rate_a, P.rate_a), P.a_min, P.a_max);
                }
            }
            if (CAND == CAND_TRACK) {          // lane - 1: row i - 1 of the same scenario.  Every lane takes part in the exchange
                const double below = __shfl_up(a, 1, 64);      // whatever its own flag says: the lane above it reads what it holds
                twin = twin && (a == below);
            }
            g = fmax(g, fmax(P.v_min - v, v - P.v_max));                             // mpc.py:316-317 (k < N)
            if (k == P.N - 1) viol |= terminal_viol_x8(P, v, a, cinf);               // mpc.py:177-180
            const double vn = fma(P.dt, a, v);
            travel += fmax(fabs(v), fabs(vn));           // sum_k max(|v_k|, |v_k+1|): what the incumbent bound lets the row still gain
            v = vn;
        }
        // (igt_fast64.h BOUND reads it instead of rolling the recurrence ahead once more at the start of every unit: with the speed
        // cap in the targets that preamble had grown to a third of a pruned unit's instructions)
        if (CAND == CAND_TRACK && row_rem) row_rem[(size_t)b * P.G + i] = travel;
        // A tracking row whose N accelerations are, bit for bit, those of the row below it (both ride the speed cap, the envelope
        // or a box limit) rolls the same G candidates again: same trajectories, same costs, and the arg-min's tie rule gives them
        // to the lower index anyway -- the row is left out.  (With the speed cap the rows above the one that just reaches v_max
        // are all such twins; before it they failed the speed box and were left out for that.)
        live = !(g > P.tol) && viol == 0 && !twin;
    }
    const unsigned long long m = __ballot(live);
    if (b < B && i == 0) {
        row_mask[b] = (m >> (lane & ~(P.G - 1))) & (P.G >= 64 ? ~0ull : ((1ull << P.G) - 1ull));
        row_mask[B + b] = cost_key((double)INFINITY);      // the scenario's incumbent of this pass, behind the masks (PartJTail): none yet
    }
}

// The search kernels' view of what part_J holds behind the partials (igt_launch.h PartJTail).  DEV_LAUNCH_LIVE_ROWS: the masks
// of accel_rows_kernel are in use, and with them the incumbents ([B] keys, set to "none" by accel_rows_kernel) and the rows'
// travel sums ([B G], tracking family).  DEV_LAUNCH_CKPT: the search pass leaves the unit winners' horizon checkpoints
// ([B W][CK_RECORD] doubles) for emit_seg_f64_kernel.
__device__ __forceinline__ const unsigned long long* live_rows_of(const KP& P, int B, int W, double* part_J) {
    return (P.dev & DEV_LAUNCH_LIVE_ROWS) ? PartJTail<double>(part_J, B, W, P.G).masks() : nullptr;
}
template <int CAND, bool VALUE>
__device__ __forceinline__ unsigned long long* incumbents_of(const KP& P, int B, int W, double* part_J) {
    return (CAND == CAND_TRACK && !VALUE && (P.dev & DEV_LAUNCH_LIVE_ROWS) && !(P.dev & (DEV_NO_BOUND | DEV_STEER_SLICES)))
               ? PartJTail<double>(part_J, B, W, P.G).incumbents() : nullptr;
}
constexpr int CK_RECORD = (f64::CK_PARTS - 1) * f64::CK_FIELDS;
static_assert(CK_RECORD == CK_RECORD_DOUBLES, "PartJTail sizes the checkpoint records");
__device__ __forceinline__ double* row_rems_of(const KP& P, int B, int W, double* part_J) {
    return PartJTail<double>(part_J, B, W, P.G).row_rems();
}
__device__ __forceinline__ double* checkpoints_of(const KP& P, int B, int W, double* part_J) {
    return (P.dev & DEV_LAUNCH_CKPT) ? PartJTail<double>(part_J, B, W, P.G).ck_records() : nullptr;
}
// queue items in unit-rank-major order when the tracking family's incumbents are in use and no order table was built
__device__ __forceinline__ bool rank_major_items(const KP& P, int cand, bool value) {
    return cand == CAND_TRACK && !value && (P.dev & DEV_LAUNCH_LIVE_ROWS) && !(P.dev & (DEV_NO_BOUND | DEV_STEER_SLICES));
}

#define IGT_SEARCH64_ARGS                                                                                            \
    KP P, int B, int W, int queues, unsigned* __restrict__ work_counter, const unsigned* __restrict__ order,          \
        int order_stride, const double* __restrict__ x0, const double* __restrict__ u_prev,                          \
        const double* __restrict__ kparams, const uint32_t* __restrict__ flags, const double* __restrict__ obs,      \
        const double* __restrict__ table, const double* __restrict__ cinf, Centre<double> cpar,          \
        double* __restrict__ part_J, int32_t* __restrict__ part_c, double* __restrict__ rec_sN,                      \
        double* __restrict__ rec_vN, double* __restrict__ rec_J, uint32_t* __restrict__ rec_viol,                    \
        unsigned* __restrict__ rec_count, int32_t* __restrict__ rec_b, int2* __restrict__ unit_seg

// One work unit = one (scenario, 64-candidate slice), rolled by one wave; leaves the slice's best (J, c), or -- value-net
// cost -- every candidate's record for value_kernel<double> (mpc.py:369).
// BOX (search_box_f64_kernel): `obs` is the poses [B,n_obs,3,N+1] and the collision verdict is the rectangle one of *box
// (igt_fast64.h ROLL_BOX) -- the unit lays out its scenario's table in LDS and rolls with it as S.obs.
template <int CAND, bool HI, bool VALUE, int NRK = 0, bool CAPTURE = false, bool BOX = false>
__device__ __forceinline__ void search_unit64(const KP& P, int W, int b, int p, const double* __restrict__ x0,
                                              const double* __restrict__ u_prev, const double* __restrict__ kparams,
                                              const uint32_t* __restrict__ flags, const double* __restrict__ obs,
                                              const double* __restrict__ table, const double* __restrict__ cinf,
                                              Centre<double> cpar, double* __restrict__ part_J,
                                              int32_t* __restrict__ part_c, double* __restrict__ rec_sN,
                                              double* __restrict__ rec_vN, double* __restrict__ rec_J,
                                              uint32_t* __restrict__ rec_viol, unsigned* __restrict__ rec_count,
                                              int32_t* __restrict__ rec_b, int2* __restrict__ unit_seg,
                                              const unsigned long long* __restrict__ row_mask = nullptr,
                                              double* __restrict__ traj = nullptr, unsigned long long* inc_all = nullptr,
                                              double* __restrict__ ck_all = nullptr, const double* __restrict__ rem_all = nullptr,
                                              const BoxModel* box = nullptr) {
    static_assert(!(BOX && CAPTURE), "the rectangle verdict: the plain units only");
    const int lane = threadIdx.x & 63;
    unsigned long long* inc = inc_all ? inc_all + b : nullptr;
    const double* rem_rows = (inc_all && rem_all) ? rem_all + (size_t)b * P.G : nullptr;
    const UnitLayout L = unit_layout(P, W, CAND, row_mask ? row_mask[b] : ~0ull);
    if (p >= L.n_units) {             // the scenario's live rows fit fewer units: this slice holds nothing
        if (lane == 0) {
            if (VALUE) unit_seg[b * W + p] = make_int2((b * W + p) * 64, 0);
            else { part_J[b * W + p] = 0.0; part_c[b * W + p] = -1; }
        }
        return;
    }
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
    NullSink sink;
    __shared__ int rank2row[64];
    rows_by_rank(L, lane, rank2row);
    int col = 0, r_first = 0, nj = 1;                        // steering slices: the unit's columns, the lane's among them
    const int c = unit_candidate(P, L, p, lane, rank2row, &col);   // -1: a lane without a candidate (rolls one, counts as lost)
    if (L.kind >= 2) unit_columns(P, L, p, r_first, nj);
    double J, sN, vN;
    unsigned viol;
    double* ck_lds = nullptr;
    if constexpr (CAPTURE) {      // small batches: every lane's trajectory is kept for emit_gather_f64_kernel (all rows, so no
                                  // Cartesian skip; same arithmetic as below, same bits)
        CaptureSink keep{traj + (size_t)(b * W + p) * traj_unit_doubles(P.N) + lane, P.N + 1};
        if (L.kind >= 2 && steer_table_fits(P, W, CAND)) {
            __shared__ double stabc[f64::STAB_MAX_ENTRIES * 3];
            f64::fill_steer_table<CAND>(P, S, nj, r_first, lane, P.lr_ratio, stabc);
            f64::rollout_one<CAND, HI, ROLL_SEARCH | ROLL_STEER_TABLE, NRK>(P, S, c, table, cinf, keep, J, viol, sN, vN, stabc + col * 3,
                                                                            nj * 3);
            __syncthreads();
        } else {
            f64::rollout_one<CAND, HI, ROLL_SEARCH, NRK>(P, S, c, table, cinf, keep, J, viol, sN, vN);
        }
    } else {
    // steering slices of the families with state-independent steering: the slice's G/W steering columns are laid out in
    // LDS once per unit instead of being recomputed by each of their 64 W/G lanes at every step (igt_fast64.h)
    // 70 % of the benchmark's scenarios: the other vehicle is out of reach over the whole horizon (or filter_preds moved it
    // away), so the unit rolls without the Cartesian rows -- a sixth of the control step's instructions
    bool far_box = false;
    if constexpr (BOX) {      // the poses of the scenario: out of reach by the rectangles' gate, or the table (nothing leaves checkpoints)
        __shared__ double boxtab[BOX_TAB_DOUBLES];
        const double* pose = obs + (size_t)b * P.n_obs * 3 * (P.N + 1);
        far_box = !(P.dev & DEV_NO_FAR) && f64::box_out_of_reach(P, S, *box, pose, lane);
        if (!far_box) f64::fill_box_table(P, *box, pose, lane, boxtab);
        S.obs = boxtab;
    }
    const bool far = BOX ? far_box : !(P.dev & DEV_NO_FAR) && obstacles_out_of_reach<double>(P, S, lane);
    // horizon checkpoints of every lane in LDS (igt_fast64.h ROLL_LEAVE_CKPT); the unit winner's go to HBM below
    constexpr unsigned UNIT = ROLL_SEARCH | ((VALUE || BOX) ? 0u : ROLL_LEAVE_CKPT) | (BOX ? ROLL_BOX : 0u);
    constexpr int CKF = f64::ck_fields(CAND);
    __shared__ double ckl[(VALUE || BOX) ? 1 : (f64::CK_PARTS - 1) * CKF * 64];
    ck_lds = (!VALUE && ck_all) ? ckl + lane : nullptr;
    if (L.kind >= 2 && steer_table_fits(P, W, CAND)) {
        __shared__ double stab[f64::STAB_MAX_ENTRIES * 3];
        f64::fill_steer_table<CAND>(P, S, nj, r_first, lane, P.lr_ratio, stab);
        if (far)
            f64::rollout_one<CAND, HI, UNIT | ROLL_STEER_TABLE | ROLL_NO_XY, NRK>(P, S, c, table, cinf, sink, J, viol, sN, vN,
                                                                                  stab + col * 3, nj * 3, nullptr, ck_lds);
        else
            f64::rollout_one<CAND, HI, UNIT | ROLL_STEER_TABLE, NRK>(P, S, c, table, cinf, sink, J, viol, sN, vN, stab + col * 3,
                                                                     nj * 3, nullptr, ck_lds);
        __syncthreads();                                  // the next unit of this wave rewrites the table
    } else if (far) {
        f64::rollout_one<CAND, HI, UNIT | ROLL_NO_XY, NRK>(P, S, c, table, cinf, sink, J, viol, sN, vN, nullptr, 0, inc, ck_lds, 0, 0, rem_rows);
    } else {
        f64::rollout_one<CAND, HI, UNIT, NRK>(P, S, c, table, cinf, sink, J, viol, sN, vN, nullptr, 0, inc, ck_lds, 0, 0, rem_rows);
    }
    }
    if (VALUE) {   // terminal value network (mpc.py:369): append the feasible candidates for value_mfma_f64_kernel; the
                   // unit's entries are contiguous, unit_seg remembers where (unit_reduce_kernel picks the unit's best)
        // The unit's entries go to the unit's own 64 slots: no counter is shared between the units (a returning atomicAdd on
        // one address retires every 11.4 ns on this part -- 262 144 units at B = 65 536 would queue for 3 ms); the dense list
        // the network runs over is built afterwards from the units' counts (value_select_kernel).
        const bool ok = viol == 0 && finite_d(J);
        const unsigned long long m = __ballot(ok);
        const unsigned n = __popcll(m);
        const unsigned base = (unsigned)(b * W + p) * 64u;
        if (ok) {
            const unsigned e = base + __popcll(m & ((1ull << lane) - 1ull));
            rec_b[e] = b; reinterpret_cast<int32_t*>(rec_viol)[e] = c; rec_sN[e] = sN; rec_vN[e] = vN; rec_J[e] = J;
        }
        if (lane == 0) unit_seg[b * W + p] = make_int2((int)base, (int)n);
        return;
    }
    const double Jq = J - (sN - S.x0[2]);                       // mpc.py:372
    double bestJ = Jq;
    int bestC = ((viol == 0) && finite_d(Jq)) ? c : -1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {                   // wave_argmin (igt_device.h) written out: it must agree with it
        const double oJ = __shfl_xor(bestJ, off, 64);
        const int oC = __shfl_xor(bestC, off, 64);
        const bool take = (oC >= 0) && (bestC < 0 || oJ < bestJ || (oJ == bestJ && oC < bestC));
        if (take) { bestJ = oJ; bestC = oC; }
    }
    if (ck_lds && bestC >= 0 && c == bestC) {          // the unit winner's lane: its checkpoints -> HBM, record [q][field]
        constexpr int CKF2 = f64::ck_fields(CAND);
        double* g = ck_all + (size_t)(b * W + p) * CK_RECORD;
#pragma unroll
        for (int q = 0; q < f64::CK_PARTS - 1; ++q)
#pragma unroll
            for (int f = 0; f < CKF2; ++f) g[q * f64::CK_FIELDS + f] = ck_lds[(size_t)(q * CKF2 + f) * 64];
    }
    if (lane == 0) {
        part_J[b * W + p] = bestJ; part_c[b * W + p] = bestC;
        // the unit's best feasible cost is the scenario's incumbent from now on (device-scope atomic: the later units of the
        // scenario may run on another XCD)
        if (inc && bestC >= 0) atomicMin(inc, cost_key(bestJ));
    }
}

// persistent waves on the per-XCD queues (search_waves), 2 or 3 per SIMD like the float kernels.  NRK = 4: the build for the
// reference's discretisation (num_rk4_steps = 4, evaluate.py:109), NRK = 0: any n_rk4 (same arithmetic, same bits)
template <int CAND, bool HI, bool VALUE, int NRK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_f64_kernel_o2(IGT_SEARCH64_ARGS) {
    search_waves(P, B, W, queues, work_counter, order, order_stride, [&](int b, int p) {
        search_unit64<CAND, HI, VALUE, NRK>(P, W, b, p, x0, u_prev, kparams, flags, obs, table, cinf, cpar, part_J, part_c, rec_sN,
                                       rec_vN, rec_J, rec_viol, rec_count, rec_b, unit_seg, live_rows_of(P, B, W, part_J), nullptr,
                                       incumbents_of<CAND, VALUE>(P, B, W, part_J), checkpoints_of(P, B, W, part_J), row_rems_of(P, B, W, part_J));
    }, rank_major_items(P, CAND, VALUE));
}
template <int CAND, bool HI, bool VALUE, int NRK>      // held to 256 registers for the tracking family (see search_fast_kernel_o2w)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_f64_kernel_o2w(IGT_SEARCH64_ARGS) {
    search_waves(P, B, W, queues, work_counter, order, order_stride, [&](int b, int p) {
        search_unit64<CAND, HI, VALUE, NRK>(P, W, b, p, x0, u_prev, kparams, flags, obs, table, cinf, cpar, part_J, part_c, rec_sN,
                                       rec_vN, rec_J, rec_viol, rec_count, rec_b, unit_seg, live_rows_of(P, B, W, part_J), nullptr,
                                       incumbents_of<CAND, VALUE>(P, B, W, part_J), checkpoints_of(P, B, W, part_J), row_rems_of(P, B, W, part_J));
    }, rank_major_items(P, CAND, VALUE));
}
// One work item = one scenario's whole pool of live lattice candidates, rolled by one wave with lanes that refill
// (igt_fast64.h rollout_pool).  Candidates are numbered as unit_candidate numbers them in the live-row layout: g = r R + q,
// column rank r from the centre outwards, q the rank among the live rows.  The steering table holds all G columns.  The item
// leaves the scenario's best (J, c) in slot 0 of its W partials, (0, -1) in the others, and with checkpoint slots the winner's
// record in slot 0: the emit kernels read the partials as they read the units'.
template <int CAND, bool HI, int NRK, bool CKPT>
__device__ __forceinline__ void search_pool64(const KP& P, int W, int b, const double* __restrict__ x0,
                                              const double* __restrict__ u_prev, const double* __restrict__ kparams,
                                              const uint32_t* __restrict__ flags, const double* __restrict__ obs,
                                              const double* __restrict__ cinf, Centre<double> cpar, double* __restrict__ part_J,
                                              int32_t* __restrict__ part_c, const unsigned long long* __restrict__ row_mask,
                                              double* __restrict__ ck_all) {
    const int lane = threadIdx.x & 63;
    const UnitLayout L = unit_layout(P, W, CAND, row_mask[b]);
    const int R = __builtin_amdgcn_readfirstlane(L.R), n = P.G * R;
    constexpr int CKF = f64::ck_fields(CAND);
    constexpr unsigned POOL = ROLL_POOL | (CKPT ? ROLL_LEAVE_CKPT : ROLL_STEP_TABLE);
    __shared__ int rank2row[64];
    // CKPT (DEV_LAUNCH_CKPT: emit in pieces): checkpoint slots and the three-double table; else no slots and the pool's table
    __shared__ double stab[f64::STAB_MAX_ENTRIES * (CKPT ? 3 : f64::POOL_STAB_FIELDS)];
    __shared__ double ckl[CKPT ? (f64::CK_PARTS - 1) * CKF * 64 : 1];
    __shared__ double rec[CKPT ? (f64::CK_PARTS - 1) * CKF : 1];
    __shared__ double start[f64::POOL_START];
    __shared__ unsigned tabw[f64::POOL_TAB];
    __shared__ double tabda[f64::POOL_TAB];
    double wJ = 0.0;
    int wC = -1;
    if (n > 0) {
        Scenario<double> S;
        load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
        rows_by_rank(L, lane, rank2row);
        if (CKPT) f64::fill_steer_table<CAND>(P, S, P.G, 0, lane, P.lr_ratio, stab);
        else f64::fill_pool_table<CAND>(P, S, P.G, lane, P.lr_ratio, stab);
        // the window of the refill table that starts at candidate number `base`: unit_candidate's numbering, cand_increments' da.
        // What it derives from R and G is derived here, behind the refill's branch, not held in registers over the control steps:
        // the empty asm makes the two opaque there.  The ISA is the check (profiles/r07_pool_loop_isa.txt): the reciprocal of R and
        // the division by G - 1 sit in the fill's block, not before the loop.  The word holds the candidate index in its low 16 bits
        // and the column rank above: C = G G <= 4096 and rank < G <= 64 (igt_api.hip validate: G divides 64).
        auto fill = [&](int base) {
            int Rf = R, Gf = P.G;
            asm volatile("" : "+s"(Rf), "+s"(Gf));
            const int lgf = __ffs(Gf) - 1;
            for (int e = lane; e < f64::POOL_TAB && base + e < n; e += 64) {
                const int g = base + e, r = small_div(g, Rf), rank = g - r * Rf;
                const int j = (r & 1) ? Gf / 2 - 1 - (r >> 1) : Gf / 2 + (r >> 1);    // unit_candidate's column order
                const int row = rank2row[rank];
                tabw[e] = (unsigned)((row << lgf) + j) | ((unsigned)r << 16);
                tabda[e] = -P.rate_a + (2 * P.rate_a) * (double)row / (double)(Gf - 1);   // cand_increments: i = c / G = row
            }
            __syncthreads();
        };
        const bool far = !(P.dev & DEV_NO_FAR) && obstacles_out_of_reach<double>(P, S, lane);
        double* ck = (CKPT && ck_all) ? ckl + lane : nullptr;
        const int stride = P.G * (CKPT ? 3 : f64::POOL_STAB_FIELDS);
        if (far) f64::rollout_pool<CAND, HI, NRK, POOL | ROLL_NO_XY>(P, S, n, fill, cinf, stab, stride, ck, rec, start, tabw, tabda, wJ, wC);
        else f64::rollout_pool<CAND, HI, NRK, POOL>(P, S, n, fill, cinf, stab, stride, ck, rec, start, tabw, tabda, wJ, wC);
        __syncthreads();                                  // rec is complete; the next item of this wave rewrites the tables
    }
    if (lane < W) {
        part_J[b * W + lane] = lane == 0 ? wJ : 0.0;
        part_c[b * W + lane] = lane == 0 ? wC : -1;
    }
    if (CKPT && ck_all && wC >= 0 && lane < CKF * (f64::CK_PARTS - 1)) {
        const int q = lane / CKF, f = lane - q * CKF;
        ck_all[(size_t)(b * W) * CK_RECORD + q * f64::CK_FIELDS + f] = rec[lane];
    }
}
template <int CAND, bool HI, bool VALUE, int NRK, bool CKPT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_f64_kernel_pool(IGT_SEARCH64_ARGS) {
    if constexpr (CAND == CAND_LATTICE && !VALUE) {
        search_waves(P, B, 1, queues, work_counter, order, order_stride, [&](int b, int) {
            search_pool64<CAND, HI, NRK, CKPT>(P, W, b, x0, u_prev, kparams, flags, obs, cinf, cpar, part_J, part_c,
                                               live_rows_of(P, B, W, part_J), CKPT ? checkpoints_of(P, B, W, part_J) : nullptr);
        });
    }
}
// small batches (captures_trajectories): the same search, every unit also leaves its 64 trajectories in `traj`
template <int CAND, bool VALUE>
__global__ __launch_bounds__(64) void search_f64_kernel_cap(IGT_SEARCH64_ARGS, double* __restrict__ traj) {
    if (queues == 0) {      // every unit has a wave of its own (search_is_static): no queues, no counters
        search_unit64<CAND, false, VALUE, 4, true>(P, W, (int)(blockIdx.x / (unsigned)W), (int)(blockIdx.x % (unsigned)W), x0, u_prev,
                                                   kparams, flags, obs, table, cinf, cpar, part_J, part_c, rec_sN, rec_vN, rec_J,
                                                   rec_viol, rec_count, rec_b, unit_seg, nullptr, traj);
        return;
    }
    search_waves(P, B, W, queues, work_counter, order, order_stride, [&](int b, int p) {
        search_unit64<CAND, false, VALUE, 4, true>(P, W, b, p, x0, u_prev, kparams, flags, obs, table, cinf, cpar, part_J, part_c,
                                                   rec_sN, rec_vN, rec_J, rec_viol, rec_count, rec_b, unit_seg, nullptr, traj);
    });
}
// ---- per-scenario candidate sets U[B,C,2,N] (igt_solve_candidates_f64; igt_launch.h plan_candidates64) ----
// The table family, every scenario with a table of its own: U[b] = U + b cand_table_doubles(C, N).  One wave per (scenario,
// 64-candidate unit) on a plain grid, the unit being candidates 64 p .. 64 p + 63 in index order (unit_layout kind 0).
//
// Staged (progress cost, N <= CAND_STAGE_ROWS / 2).  The unit's slab is 2 N 64 contiguous doubles, candidate-major: entry r of
// candidate j at slab[j 2 N + r].  The wave lays it out in LDS as columns, cols[r 64 + j] -- polish_f64_kernel's layout -- and
// rolls with rollout_one on the table family, the lane's column as its table (ROLL_STEER_TABLE): the statements of every other
// roll-out, so the bits of the shared table's solve.  Every byte of U crosses HBM once; the control-step loop reads LDS
// (ds_read_b64 of cols[k 64 + lane]: 64 consecutive doubles, no two lanes on one bank in a pass).
// The copy.  A ds_write_b64 of cols[r 64 + j] lands on banks (128 r + 2 j) % 32 = 2 (j % 16) and the one above: the row does not
// count, 512 B being a multiple of the 128 B the banks span, only the candidate does.  A straight transpose of a coalesced load
// (lane = consecutive r of one candidate) would put a pass's 16 lanes on ONE bank pair, 16-way.  Here lane l of trip (rb, q)
// takes candidate 16 q + (l & 15), row 4 rb + (l >> 4): the 16 lanes of a pass hold 16 different candidates modulo 16 -- all 32
// banks once, no conflict -- and the load they come from reads four 32-byte pieces per candidate, sixteen candidates 16 N bytes
// apart: sectors, not lines, but every sector it touches is used whole across the four lane groups of the same instruction.
// All trips' loads are issued before the first store (the bounds are constants, a row past 2 N is loaded from row 2 N - 1 and
// not stored): up to 40 loads in flight per lane, in registers that the roll-out has not claimed yet.
// LDS: CAND_STAGE_ROWS rows of 512 B, 20 KB whatever N is: eight waves fill a compute unit's 160 KB, and two waves per SIMD is
// what the roll-out's registers allow anyway.
constexpr int CAND_STAGE_ROWS = (int)(CAND_SLAB_MAX_BYTES / (64 * sizeof(double)));      // 40: horizons up to N = 20
template <bool HI, int NRK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_cand_staged_f64_kernel(
        KP P, int B, int W, const double* __restrict__ x0, const double* __restrict__ u_prev, const double* __restrict__ kparams,
        const uint32_t* __restrict__ flags, const double* __restrict__ obs, const double* __restrict__ U,
        const double* __restrict__ cinf, double* __restrict__ part_J, int32_t* __restrict__ part_c) {
    __shared__ double cols[CAND_STAGE_ROWS * 64];
    const int b = (int)(blockIdx.x / (unsigned)W), p = (int)(blockIdx.x % (unsigned)W), lane = threadIdx.x;
    if (b >= B) return;
    const int n2 = 2 * P.N;                                   // <= CAND_STAGE_ROWS (plan_candidates64)
    const double* __restrict__ slab = U + ((size_t)b * P.C + (size_t)p * 64) * n2;
    {
        constexpr int TRIPS = CAND_STAGE_ROWS / 4;
        const int j = lane & 15, r0 = lane >> 4;
        double held[TRIPS][4];
#pragma unroll
        for (int rb = 0; rb < TRIPS; ++rb) {
            const int r = 4 * rb + r0, rr = r < n2 ? r : n2 - 1;
#pragma unroll
            for (int q = 0; q < 4; ++q) held[rb][q] = slab[(size_t)(16 * q + j) * n2 + rr];
        }
#pragma unroll
        for (int rb = 0; rb < TRIPS; ++rb) {
            const int r = 4 * rb + r0;
            if (r < n2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) cols[r * 64 + 16 * q + j] = held[rb][q];
            }
        }
    }
    __syncthreads();
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs);
    const bool far = !(P.dev & DEV_NO_FAR) && obstacles_out_of_reach<double>(P, S, lane);
    NullSink sink;
    const int c = p * 64 + lane;
    double J, sN, vN;
    unsigned viol;
    if (far) f64::rollout_one<CAND_TABLE, HI, ROLL_SEARCH | ROLL_STEER_TABLE | ROLL_NO_XY, NRK>(P, S, c, nullptr, cinf, sink, J, viol, sN, vN, cols + lane, 64);
    else f64::rollout_one<CAND_TABLE, HI, ROLL_SEARCH | ROLL_STEER_TABLE, NRK>(P, S, c, nullptr, cinf, sink, J, viol, sN, vN, cols + lane, 64);
    // what search_unit64 leaves for a unit without checkpoint slots or an incumbent: its statements
    const double Jq = J - (sN - S.x0[2]);                       // mpc.py:372
    double bestJ = Jq;
    int bestC = ((viol == 0) && finite_d(Jq)) ? c : -1;
    wave_argmin(bestJ, bestC);
    if (lane == 0) { part_J[b * W + p] = bestJ; part_c[b * W + p] = bestC; }
}
// Direct (horizons whose slab does not fit; the value-network cost, whose units leave records): search_unit64 itself, its
// table the scenario's own, read from HBM step by step as the shared table is read from L2.
template <bool HI, bool VALUE, int NRK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_cand_direct_f64_kernel(IGT_SEARCH64_ARGS) {
    const int b = (int)(blockIdx.x / (unsigned)W), p = (int)(blockIdx.x % (unsigned)W);
    if (b >= B) return;
    search_unit64<CAND_TABLE, HI, VALUE, NRK>(P, W, b, p, x0, u_prev, kparams, flags, obs, scenario_table(P, table, b, true),
                                              cinf, cpar, part_J, part_c, rec_sN, rec_vN, rec_J, rec_viol, rec_count, rec_b, unit_seg);
}
// ---- the rectangle (OBCA) collision model (igt_solve_batch_box_f64; igt_launch.h plan_box64) ----
// search_unit64 with the rectangle verdict, one wave per (scenario, 64-candidate unit) on a plain grid as the direct kernel
// above: no queues, no pool, no prelude, every acceleration row, the partials (or the value network's records) as the only
// workspace.  The generic sub-step build alone (NRK = 0: any n_rk4, the same bits as the unrolled one): 16 kernels, not 24.
template <int CAND, bool HI, bool VALUE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_box_f64_kernel(IGT_SEARCH64_ARGS, BoxModel box) {
    const int b = (int)(blockIdx.x / (unsigned)W), p = (int)(blockIdx.x % (unsigned)W);
    if (b >= B) return;
    search_unit64<CAND, HI, VALUE, 0, false, true>(P, W, b, p, x0, u_prev, kparams, flags, obs, table, cinf, cpar, part_J, part_c, rec_sN,
                                                   rec_vN, rec_J, rec_viol, rec_count, rec_b, unit_seg, nullptr, nullptr, nullptr, nullptr,
                                                   nullptr, &box);
}
// one 64-thread block per scenario: final arg-min over the W partials, then the winner's trajectory copied out of the unit
// that rolled it.  Which lane that was is asked of unit_candidate itself, so the two cannot drift apart.
template <int CAND>
__global__ __launch_bounds__(64) void emit_gather_f64_kernel(KP P, int B, int W, const double* __restrict__ x0,
                                                             const double* __restrict__ u_prev,
                                                             const uint32_t* __restrict__ flags, Centre<double> cpar,
                                                             const double* __restrict__ part_J,
                                                             const int32_t* __restrict__ part_c,
                                                             const double* __restrict__ traj, double* __restrict__ cost_out,
                                                             int32_t* __restrict__ argmin_out, int32_t* __restrict__ status_out,
                                                             double* __restrict__ x_out, double* __restrict__ u_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double bestJ = 0.0;
    int c = -1, pw = 0;
    for (int w = 0; w < W; ++w) {      // best_partial (igt_kernels_common.h) written out: it must agree with it
        const int cw = part_c[(size_t)b * W + w];
        const double Jw = part_J[(size_t)b * W + w];
        if (cw >= 0 && (c < 0 || Jw < bestJ || (Jw == bestJ && cw < c))) { bestJ = Jw; c = cw; pw = w; }
    }
    if (c >= 0 && inputs_refused<double>(P, b, x0, u_prev, flags, cpar)) c = -1;
    if (lane == 0) {
        cost_out[b] = c >= 0 ? bestJ : (double)INFINITY;
        argmin_out[b] = c;
        status_out[b] = c >= 0 ? 0 : 1;
    }
    const int N1 = P.N + 1, nx = 7 * N1, nu = 2 * P.N;
    double* xo = x_out + (size_t)b * nx;
    double* uo = u_out + (size_t)b * nu;
    const UnitLayout L = unit_layout(P, W, CAND, ~0ull);      // batches that keep trajectories run the full layout
    const unsigned long long holder = __ballot(c >= 0 && unit_candidate(P, L, pw, lane, nullptr) == c);
    if (c < 0 || holder == 0ull) {     // is_opt False (mpc.py:402-406): no trajectory
        for (int i = lane; i < nx; i += 64) xo[i] = (double)NAN;
        for (int i = lane; i < nu; i += 64) uo[i] = (double)NAN;
        return;
    }
    const double* src = traj + (size_t)(b * W + pw) * traj_unit_doubles(P.N) + (__ffsll((long long)holder) - 1);
    for (int i = lane; i < nx; i += 64) xo[i] = src[(size_t)i * 64];
    for (int i = lane; i < nu; i += 64) uo[i] = src[(size_t)((7 + i / P.N) * N1 + i % P.N) * 64];
}
#if IGT_DEV_KERNELS
template <int CAND, bool HI, bool VALUE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void search_f64_kernel_o3(IGT_SEARCH64_ARGS) {
    search_waves(P, B, W, queues, work_counter, order, order_stride, [&](int b, int p) {
        search_unit64<CAND, HI, VALUE>(P, W, b, p, x0, u_prev, kparams, flags, obs, table, cinf, cpar, part_J, part_c, rec_sN,
                                       rec_vN, rec_J, rec_viol, rec_count, rec_b, unit_seg, live_rows_of(P, B, W, part_J));
    });
}
#endif

// one lane per scenario: final arg-min over the W partials, then the winner re-rolled with the same arithmetic
// (general sub-step variant: the lanes of the wave belong to different scenarios) -> x*[7,N+1], u*[2,N]
// PRIO > 0 (igt_launch.h plan_search64 emit_priority): beside resident search waves this wave is the youngest on its SIMD and gets
// the issue slots they leave; it raises its priority once, before anything else, and keeps it.  A build of its own, not a
// run-time condition: s_setprio ignores EXEC and must not sit under a branch the compiler cannot prove wave-uniform, and the
// PRIO = 0 build stays the code it was.
// OWN (the per-scenario candidate sets): `table` is U[B,C,2,N] and the scenario rolls from its own part of it.
template <int CAND, bool HI, int NRK, int PRIO = 0, bool OWN = false>
__global__ __launch_bounds__(64) void emit_f64_kernel(KP P, int B, int W, const double* __restrict__ x0,
                                                      const double* __restrict__ u_prev,
                                                      const double* __restrict__ kparams,
                                                      const uint32_t* __restrict__ flags, const double* __restrict__ obs,
                                                      const double* __restrict__ table, const double* __restrict__ cinf,
                                                      Centre<double> cpar, const double* __restrict__ part_J,
                                                      const int32_t* __restrict__ part_c, double* __restrict__ cost_out,
                                                      int32_t* __restrict__ argmin_out, int32_t* __restrict__ status_out,
                                                      double* __restrict__ x_out, double* __restrict__ u_out) {
    if constexpr (PRIO > 0) __builtin_amdgcn_s_setprio(PRIO);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double bestJ = 0.0;
    int c = -1;
    for (int w = 0; w < W; ++w) {      // best_partial (igt_kernels_common.h) written out: it must agree with it
        const int cw = part_c[(size_t)b * W + w];
        const double Jw = part_J[(size_t)b * W + w];
        if (cw >= 0 && (c < 0 || Jw < bestJ || (Jw == bestJ && cw < c))) { bestJ = Jw; c = cw; }
    }
    if (c >= 0 && inputs_refused<double>(P, b, x0, u_prev, flags, cpar)) c = -1;
    write_verdict<double>(b, bestJ, c, cost_out, argmin_out, status_out);
    double* xo = x_out + (size_t)b * 7 * (P.N + 1);
    double* uo = u_out + (size_t)b * 2 * P.N;
    if (c < 0) { no_trajectory<double>(P, xo, uo); return; }
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
    StoreSink<double> sink{xo, uo, P.N};
    double J, sN, vN;
    unsigned viol;
    f64::rollout_one<CAND, HI, ROLL_EMIT, NRK>(P, S, c, scenario_table(P, table, b, OWN), cinf, sink, J, viol, sN, vN);
}

// ---- emit in pieces (batches that do not keep trajectories; progress cost) ----
// One roll-out is a serial chain, and a wave issues a float64 instruction every four cycles however few of its lanes are
// active: emit_f64_kernel's 64 waves at B = 4096 take one roll-out of time, 51 us.  Here a workgroup of four waves owns S
// scenarios (lane = scenario): wave w rolls steps [w N / 4, (w + 1) N / 4) of each winner's Frenet rows from the checkpoint the
// search pass left (igt_fast64.h ROLL_RESUME) into LDS -- states, controls and (sin, cos)(beta_k) -- , then the first wave rolls the
// Cartesian rows x, y, psi from those controls (cartesian_rows), and the workgroup writes its scenarios' x*[7, N+1] and u*[2, N]
// out of LDS as they lie in HBM: contiguous, every store of a wave a full line (emit_f64_kernel: one lane per scenario,
// 64 lines touched per store instruction, 2.6x the bytes at B = 65 536).  The same statements on the same numbers as the
// roll-out in one piece: bit-identical (tests: against IGT_DEV_FLAGS = 16777216 and against rollout-all).
struct SegSink {
    static constexpr bool kKeepsStates = true;
    double* X;      // this scenario's [7][N+1] in LDS
    double* U;      // [2][N]
    double* SB;     // [N] sin beta_k
    double* CB;     // [N] cos beta_k
    int N1;
    __device__ __forceinline__ void ctrl(int, int k, double a, double df) { U[k] = a; U[N1 - 1 + k] = df; }
    __device__ __forceinline__ void slip(int, int k, double sb, double cb) { SB[k] = sb; CB[k] = cb; }
    __device__ __forceinline__ void state(int, int k, const double (&st)[7]) {
        X[2 * N1 + k] = st[2]; X[3 * N1 + k] = st[3]; X[4 * N1 + k] = st[4]; X[5 * N1 + k] = st[5];
        if (k == 0) { X[0] = st[0]; X[N1] = st[1]; X[6 * N1] = st[6]; }
    }
};

struct LdsControls {         // tracking family: the controls of step k as the Frenet pieces left them in LDS
    const double* A; const double* SB; const double* CB;
    __device__ __forceinline__ void operator()(int k, double& a, double& sb, double& cb) const { a = A[k]; sb = SB[k]; cb = CB[k]; }
};
constexpr int SEG_THREADS = 320;      // four waves for the pieces + one for the Cartesian rows (idle in the tracking family's first phase)

template <int CAND, bool HI, int NRK>
__global__ __launch_bounds__(SEG_THREADS) void emit_seg_f64_kernel(KP P, int B, int W, int S, const double* __restrict__ x0,
                                                           const double* __restrict__ u_prev, const double* __restrict__ kparams,
                                                           const uint32_t* __restrict__ flags, const double* __restrict__ obs,
                                                           const double* __restrict__ table, const double* __restrict__ cinf,
                                                           Centre<double> cpar, const double* __restrict__ part_J,
                                                           const int32_t* __restrict__ part_c, double* __restrict__ ck_all,
                                                           double* __restrict__ cost_out, int32_t* __restrict__ argmin_out,
                                                           int32_t* __restrict__ status_out, double* __restrict__ x_out,
                                                           double* __restrict__ u_out) {
    extern __shared__ double seg_lds[];
    __shared__ int win[64];
    const int N1 = P.N + 1, per = seg_doubles_per_scenario(P.N);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b0 = blockIdx.x * S, b = b0 + lane;
    const bool active = lane < S && b < B;
    double bestJ = 0.0;
    int c = -1, pw = 0;
    if (active) {
        for (int w = 0; w < W; ++w) {      // best_partial (igt_kernels_common.h) written out: it must agree with it
            const int cw = part_c[(size_t)b * W + w];
            const double Jw = part_J[(size_t)b * W + w];
            if (cw >= 0 && (c < 0 || Jw < bestJ || (Jw == bestJ && cw < c))) { bestJ = Jw; c = cw; pw = w; }
        }
        if (c >= 0 && inputs_refused<double>(P, b, x0, u_prev, flags, cpar)) c = -1;
        if (wave == 0) {
            write_verdict<double>(b, bestJ, c, cost_out, argmin_out, status_out);
            win[lane] = c;
        }
    }
    double* blk = seg_lds + (size_t)(lane < S ? lane : 0) * per;
    Scenario<double> Sc;
    if (active && c >= 0) {
        load_scenario<double>(Sc, P, b, x0, u_prev, kparams, flags, obs, cpar);
        if (wave < f64::CK_PARTS) {
            SegSink sink{blk, blk + 7 * N1, blk + 7 * N1 + 2 * P.N, blk + 7 * N1 + 3 * P.N, N1};
            const int k0 = f64::ckpt_step(P.N, wave), k1 = f64::ckpt_step(P.N, wave + 1);
            double* ck = wave > 0 ? ck_all + ((size_t)b * W + pw) * CK_RECORD + (size_t)(wave - 1) * f64::CK_FIELDS : nullptr;
            double J, sN, vN;
            unsigned viol;
            f64::rollout_one<CAND, HI, ROLL_EMIT_PIECE | ROLL_NO_XY, NRK>(P, Sc, c, table, cinf, sink, J, viol, sN, vN, nullptr, 0, nullptr, ck, k0, k1);
        } else if (CAND != CAND_TRACK) {      // beside the pieces: the Cartesian rows, the controls generated on the spot
            f64::StepControls<CAND> ctl(P, Sc, c, table);
            f64::cartesian_rows<HI, NRK>(P, Sc.x0[0], Sc.x0[1], Sc.x0[6], Sc.x0[5], ctl, blk, blk + N1, blk + 6 * N1, 1);
        }
    }
    __syncthreads();
    if (CAND == CAND_TRACK) {                  // behind the pieces: the steering is theirs to decide
        if (wave == f64::CK_PARTS && active && c >= 0) {
            LdsControls ctl{blk + 7 * N1, blk + 7 * N1 + 2 * P.N, blk + 7 * N1 + 3 * P.N};
            f64::cartesian_rows<HI, NRK>(P, Sc.x0[0], Sc.x0[1], Sc.x0[6], Sc.x0[5], ctl, blk, blk + N1, blk + 6 * N1, 1);
        }
        __syncthreads();
    }
    // the workgroup's scenarios as they lie in HBM (is_opt False, mpc.py:402-406: NaN)
    const int nS = B - b0 < S ? B - b0 : S, nx = 7 * N1, nu = 2 * P.N;
    double* xo = x_out + (size_t)b0 * nx;
    double* uo = u_out + (size_t)b0 * nu;
    for (int i = threadIdx.x; i < nS * nx; i += SEG_THREADS) {
        const int sc = i / nx, r = i - sc * nx;
        xo[i] = win[sc] >= 0 ? seg_lds[(size_t)sc * per + r] : (double)NAN;
    }
    for (int i = threadIdx.x; i < nS * nu; i += SEG_THREADS) {
        const int sc = i / nu, r = i - sc * nu;
        uo[i] = win[sc] >= 0 ? seg_lds[(size_t)sc * per + nx + r] : (double)NAN;
    }
}

// ---- polish of the winner (igt_params.polish_iters; float64, progress cost) ----
// One wave per solved scenario improves the emitted plan u*[2, N] by projected-gradient steps.  An iteration is two kinds of
// trips of 64 roll-outs, one per lane: the forward-difference gradient (perturbation c = row c / N, step c % N on lane c; one trip
// for N <= 32, two up to IGT_MAX_N), then the line search (trial m on lane m: u + 2^(-m/3) d, clamped step by step to the rate
// window around the clamped step before it and to the input box).  Every lane's control sequence lies in LDS, [2 N][64]: the 64
// lanes' reads of step k are 64 consecutive doubles, no two on one bank in a pass.  The roll-out is rollout_one itself on the
// table family with the lane's LDS column as its table (ROLL_STEER_TABLE): the statements of search, emit and rollout-all, so
// cost and verdicts of a trial are the bits igt_rollout_batch_f64 gives for the same controls, and since all lanes belong to one
// scenario the sub-step variants are voted as in a search unit.  Scenarios whose obstacles are out of reach roll the trips
// without the Cartesian rows (obstacles_out_of_reach).  A plan that changed is rolled once more with all rows into LDS and
// written back as whole rows; one that did not is left alone.  No workspace, no host synchronisation: one launch on the stream.
// ADJ (igt_set_polish_gradient IGT_GRAD_ADJOINT): the gradient trips are replaced by the analytic gradient at the plan.  The
// plan's node states lie in xl (iteration 1: the emitted x_out); lane k forms (A_k, B_k) of control step k from them
// (igt_adjoint64.h step_jacobian -- N Jacobians side by side, a few control steps' time) into the slot region, which is idle
// until the trials are laid out; the costate recursion over the N steps is then run by every lane on the same LDS words
// (broadcast reads, ~25 fused multiply-adds a step), lane 0 keeps g.  Direction, trials, verdicts and acceptance are the
// statements of the forward-difference mode.  An accepted trial is rolled once more with all rows, every lane its own trial as
// it lies in its column, and the accepted lane keeps the states in xl: the next iteration's node states and the final
// write-back -- the roll the forward-difference mode does once at the end, moved into the loop (the sub-step variants the
// wave votes for are bit-identical where they apply, so the states are those of the plan rolled alone).  An iteration is a
// Jacobian pass, a trial trip and an accepted-plan roll against g_trips + 1 trips; the LDS is polish_lds_doubles(N) either way.
// NEWTON (igt_set_polish_step IGT_POLISH_STEP_NEWTON; an ADJ build): lane k leaves step k's Jacobian, node values and inputs in
// one record of the slot region, [N][NEWTON_REC]; every lane then runs the costate recursion and the Riccati sweep of the
// Gauss-Newton model (igt_adjoint64.h Riccati) in one backward loop over the records, broadcast reads again, lane 0 keeps g and
// leaves the gains K_k (6) and kappa_k (2) in the record.  The forward sweep dz_0 = 0, dN_k = kappa_k + K_k dz_k,
// dz_k+1 = A_k dz_k + B_k dN_k then leaves dN [2 N] behind xl -- the 2 N doubles this build's LDS grows by
// (polish_newton_lds_doubles) --, non-finite entries 0, all of it 0 if a determinant was non-finite or <= 0, the steering row 0
// when the steering rate is.  Both sweeps are a phase of their own, done before the trials are laid out: nothing of them lives
// across rollout_one.  Trials: lane m < 32 takes u + 2^(-m/3) dN (not rescaled: trial 0 is the full Newton step), lane m >= 32
// takes u + 2^(-(m-32)/3) d with d the scaled -g of the gradient modes; projection, verdicts, butterfly, acceptance and the
// accepted plan's roll are the statements above.
constexpr double POLISH_EPS = 1e-4;
__host__ __device__ inline size_t polish_lds_doubles(int N) { return (size_t)2 * N * 64 + 4 * N + 7 * (N + 1); }
__host__ __device__ inline size_t polish_newton_lds_doubles(int N) { return polish_lds_doubles(N) + 2 * N; }
constexpr int NEWTON_REC = 28;                        // doubles per step in the Newton build's records (16-byte aligned)
template <bool HI, int NRK, bool ADJ = false, bool NEWTON = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void polish_f64_kernel(
        KP P, int B, int iters, const double* __restrict__ x0, const double* __restrict__ u_prev, const double* __restrict__ kparams,
        const uint32_t* __restrict__ flags, const double* __restrict__ obs, const double* __restrict__ cinf,
        const int32_t* __restrict__ status_out, double* __restrict__ cost_out, double* __restrict__ x_out, double* __restrict__ u_out) {
    extern __shared__ double polish_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B || status_out[b] != 0) return;             // unsolved: neither read nor written
    const int N = P.N, n2 = 2 * N;
    double* slot = polish_lds;                            // [2 N][64] the lanes' control sequences
    double* u = slot + (size_t)n2 * 64;                   // [2 N] the plan so far
    double* g = u + n2;                                   // [2 N] gradient, then direction
    double* xl = g + n2;                                  // [7][N + 1] the final plan's states
    static_assert(ADJ || !NEWTON, "the Newton step is built on the adjoint build");
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs);
    const bool far = !(P.dev & DEV_NO_FAR) && obstacles_out_of_reach<double>(P, S, lane);
    for (int i = lane; i < n2; i += 64) u[i] = u_out[(size_t)b * n2 + i];
    if (ADJ) {
        for (int i = lane; i < 7 * (N + 1); i += 64) xl[i] = x_out[(size_t)b * 7 * (N + 1) + i];
    }
    double J0 = cost_out[b];
    bool changed = false;
    NullSink none;
    __syncthreads();
    const int g_trips = (n2 + 63) >> 6;
    for (int it = 0; it < iters; ++it) {
        double bestJ = 0.0;
        int bestM = -1;
        if (ADJ) {
            const int N1 = N + 1;
            adj::StepModel M;
            M.init(P, S.b0, S.b1, S.kv);
            if (lane < N) {                               // (A_k, B_k) of step k = lane, [15][N] in the slot region
                double T[3][5];
                adj::step_jacobian(M, xl[2 * N1 + lane], xl[3 * N1 + lane], xl[4 * N1 + lane], xl[5 * N1 + lane], u[lane], u[N + lane], T);
                if (NEWTON) {                             // ... NEWTON: step k's record, [N][NEWTON_REC] (see below)
                    double* rc = slot + (size_t)lane * NEWTON_REC;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int d = 0; d < 5; ++d) rc[r * 5 + d] = T[r][d];
                    rc[15] = xl[3 * N1 + lane]; rc[16] = xl[4 * N1 + lane]; rc[17] = u[lane]; rc[18] = u[N + lane];
                } else {
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int d = 0; d < 5; ++d) slot[(size_t)(r * 5 + d) * N + lane] = T[r][d];
                }
            }
            __syncthreads();
            if (NEWTON) {
                // One backward loop for the costate recursion and the Riccati sweep, one forward loop: step k's words lie in one
                // record -- T_k (15), ey_k, epsi_k, a_k, df_k (4), one free, K_k and kappa_k (8) -- so a step is one address and
                // wide broadcast reads, and the 19 words are read once for both recursions.  The addresses are formed from a
                // copy of N that the compiler cannot see through: formed from N they are hoisted out of the iteration loop and
                // held in scalar registers across both roll-outs, which shows as scratch (make resource-usage-polish).
                int Nn = N;
                asm volatile("" : "+s"(Nn));
                const int N1n = Nn + 1;
                double* dn = xl + 7 * N1n;                 // [2 N] the Newton direction
                double lam[4] = {-1.0, 2.0 * xl[3 * N1n + Nn], 2.0 * xl[4 * N1n + Nn], 0.0};
                adj::Riccati ric;
                ric.init(xl[3 * N1n + Nn], xl[4 * N1n + Nn]);
                for (int k = Nn - 1; k >= 0; --k) {
                    double* rc = slot + (size_t)k * NEWTON_REC;
                    double T[3][5], K[2][3], kap[2], ga, gd;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int d = 0; d < 5; ++d) T[r][d] = rc[r * 5 + d];
                    const double ey = rc[15], ep = rc[16], a = rc[17], df = rc[18];
                    adj::costate_step(T, P.dt, P.w_u, ey, ep, a, df, lam, ga, gd);
                    ric.step(T, P.dt, P.w_u, ey, ep, a, df, K, kap);
                    if (lane == 0) {
                        g[k] = finite_d(ga) ? ga : 0.0;
                        g[Nn + k] = finite_d(gd) ? gd : 0.0;
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
#pragma unroll
                            for (int j = 0; j < 3; ++j) rc[20 + c * 3 + j] = K[c][j];
                            rc[26 + c] = kap[c];
                        }
                    }
                }
                __syncthreads();
                const bool steer = P.rate_df > 0.0;
                double dz[3] = {0.0, 0.0, 0.0};
                for (int k = 0; k < Nn; ++k) {
                    const double* rc = slot + (size_t)k * NEWTON_REC;
                    double T[3][5], K[2][3], kap[2], d[2];
#pragma unroll
                    for (int r = 1; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 5; ++c) T[r][c] = rc[r * 5 + c];
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) K[c][j] = rc[20 + c * 3 + j];
                        kap[c] = rc[26 + c];
                    }
                    adj::newton_forward_step(T, P.dt, K, kap, steer, dz, d);
                    if (lane == 0) {
                        dn[k] = (ric.ok && finite_d(d[0])) ? d[0] : 0.0;
                        dn[Nn + k] = (ric.ok && finite_d(d[1])) ? d[1] : 0.0;
                    }
                }
            } else {                                      // (the adjoint build's own text: sharing it with NEWTON moves its code)
                double lam[4] = {-1.0, 2.0 * xl[3 * N1 + N], 2.0 * xl[4 * N1 + N], 0.0};      // d J / d (s, ey, epsi, v) at node N
                for (int k = N - 1; k >= 0; --k) {
                    double T[3][5], ga, gd;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int d = 0; d < 5; ++d) T[r][d] = slot[(size_t)(r * 5 + d) * N + k];
                    adj::costate_step(T, P.dt, P.w_u, xl[3 * N1 + k], xl[4 * N1 + k], u[k], u[N + k], lam, ga, gd);
                    if (lane == 0) {
                        g[k] = finite_d(ga) ? ga : 0.0;
                        g[N + k] = finite_d(gd) ? gd : 0.0;
                    }
                }
            }
            __syncthreads();
        }
        for (int trip = ADJ ? g_trips : 0; trip <= g_trips; ++trip) {
            const bool search = trip == g_trips;
            if (!search) {                                // u + eps e_c: no projection
                const int c = trip * 64 + lane;
                for (int i = 0; i < n2; ++i) slot[(size_t)i * 64 + lane] = i == c ? u[i] + POLISH_EPS : u[i];
            } else {
                // d = -g / scale: the longest trial moves some input by four rate limits
                double ma = 0.0, md = 0.0;
                for (int k = lane; k < N; k += 64) { ma = fmax(ma, fabs(g[k])); md = fmax(md, fabs(g[N + k])); }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    ma = fmax(ma, __shfl_xor(ma, off, 64));
                    md = fmax(md, __shfl_xor(md, off, 64));
                }
                const bool steer = P.rate_df > 0.0;
                const double scale = (steer ? fmax(ma / (4.0 * P.rate_a), md / (4.0 * P.rate_df)) : ma / (4.0 * P.rate_a)) + 1e-30;
                __syncthreads();                          // every lane has read g
                for (int i = lane; i < n2; i += 64) g[i] = (i < N || steer) ? -g[i] / scale : 0.0;
                __syncthreads();
                if (NEWTON) {                             // dN on the lower half of the lanes, the scaled -g on the upper
                    const double alpha = exp2(-(double)(lane & 31) / 3.0);
                    const double* dir = lane < 32 ? xl + 7 * (N + 1) : g;
                    double pa = S.a_prev, pd = S.df_prev;
                    for (int k = 0; k < N; ++k) {
                        pa = clampd(clampd(u[k] + alpha * dir[k], pa - P.rate_a, pa + P.rate_a), P.a_min, P.a_max);
                        pd = clampd(clampd(u[N + k] + alpha * dir[N + k], pd - P.rate_df, pd + P.rate_df), -P.df_max, P.df_max);
                        slot[(size_t)k * 64 + lane] = pa;
                        slot[(size_t)(N + k) * 64 + lane] = pd;
                    }
                } else {    // not shared with the branch above: one loop over `dir` reorders registers in the forward-difference
                            // builds, which must stay the device code they were (profiles/polish_newton_identity.txt)
                    const double alpha = exp2(-(double)lane / 3.0);
                    double pa = S.a_prev, pd = S.df_prev;
                    for (int k = 0; k < N; ++k) {
                        pa = clampd(clampd(u[k] + alpha * g[k], pa - P.rate_a, pa + P.rate_a), P.a_min, P.a_max);
                        pd = clampd(clampd(u[N + k] + alpha * g[N + k], pd - P.rate_df, pd + P.rate_df), -P.df_max, P.df_max);
                        slot[(size_t)k * 64 + lane] = pa;
                        slot[(size_t)(N + k) * 64 + lane] = pd;
                    }
                }
            }
            double J, sN, vN;
            unsigned viol;
            if (far) f64::rollout_one<CAND_TABLE, HI, ROLL_POLISH | ROLL_NO_XY, NRK>(P, S, 0, nullptr, cinf, none, J, viol, sN, vN, slot + lane, 64);
            else f64::rollout_one<CAND_TABLE, HI, ROLL_POLISH, NRK>(P, S, 0, nullptr, cinf, none, J, viol, sN, vN, slot + lane, 64);
            const double Jq = J - (sN - S.x0[2]);         // mpc.py:372
            if (!search) {
                const int c = trip * 64 + lane;
                if (c < n2) g[c] = finite_d(Jq) ? (Jq - J0) / POLISH_EPS : 0.0;
                __syncthreads();
            } else {
                bestJ = Jq;
                bestM = (viol == 0 && finite_d(Jq)) ? lane : -1;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {     // the search's butterfly on (J, m), ties to the lowest m
                    const double oJ = __shfl_xor(bestJ, off, 64);
                    const int oM = __shfl_xor(bestM, off, 64);
                    const bool take = (oM >= 0) && (bestM < 0 || oJ < bestJ || (oJ == bestJ && oM < bestM));
                    if (take) { bestJ = oJ; bestM = oM; }
                }
            }
        }
        if (bestM < 0 || !(bestJ < J0)) break;            // accepted only when feasible and strictly cheaper
        __syncthreads();
        for (int i = lane; i < n2; i += 64) u[i] = slot[(size_t)i * 64 + bestM];
        J0 = bestJ;
        changed = true;
        __syncthreads();
        if (ADJ) {                                        // the accepted trial with all rows: its lane keeps the states
            StoreSink<double> keep{lane == bestM ? xl : nullptr, nullptr, N};
            double J, sN, vN;
            unsigned viol;
            f64::rollout_one<CAND_TABLE, HI, ROLL_POLISH, NRK>(P, S, 0, nullptr, cinf, keep, J, viol, sN, vN, slot + lane, 64);
            J0 = __shfl(J - (sN - S.x0[2]), bestM, 64);
            __syncthreads();
        }
    }
    if (!changed) return;
    if (ADJ) {
        const int nx = 7 * (N + 1);
        for (int i = lane; i < nx; i += 64) x_out[(size_t)b * nx + i] = xl[i];
        for (int i = lane; i < n2; i += 64) u_out[(size_t)b * n2 + i] = u[i];
        if (lane == 0) cost_out[b] = J0;
        return;
    }
    // the polished plan with all rows: every lane rolls it (one wave's time either way), lane 0 keeps the states
    for (int i = 0; i < n2; ++i) slot[(size_t)i * 64 + lane] = u[i];
    StoreSink<double> keep{lane == 0 ? xl : nullptr, nullptr, N};
    double J, sN, vN;
    unsigned viol;
    f64::rollout_one<CAND_TABLE, HI, ROLL_POLISH, NRK>(P, S, 0, nullptr, cinf, keep, J, viol, sN, vN, slot + lane, 64);
    __syncthreads();
    const int nx = 7 * (N + 1);
    for (int i = lane; i < nx; i += 64) x_out[(size_t)b * nx + i] = xl[i];
    for (int i = lane; i < n2; i += 64) u_out[(size_t)b * n2 + i] = u[i];
    if (lane == 0) cost_out[b] = J - (sN - S.x0[2]);
}

// ---- polish of the winner under the value-network cost (igt_set_value_polish; float64, gt_mpc) ----
// J(u) = stage terms - V_out(s_N, v_N) (mpc.py:356-369): the terminal term is the network's, so an iteration cannot stay inside one
// kernel as polish_f64_kernel's does -- the network's kernels stand between its parts.  Six launches on the solve's stream, each
// sized by B alone (igt_api.hip solve_impl): the three of igt_cost_gradient_vn_f64 on u_out, value_trials_f64_kernel, the
// values-alone terminal_value_f64_kernel over the 64 B trial records, value_accept_f64_kernel.  The scratch between them is the
// solve's ValuePolishLayout (igt_value_polish_layout.h).  One wave per scenario in both kernels; a scenario is polished while
// alive[b] is set: in iteration 1 where status_out[b] == 0, afterwards where the iteration before accepted a trial.
// Trials: the gradient's non-finite entries become 0; scale, d, the 64 trials u + 2^(-m/3) d with their step-by-step clamps and
// the [2 N][64] LDS columns are polish_f64_kernel's, and so is the roll-out: rollout_one on the table family with the lane's
// column as its table (ROLL_POLISH), the sub-step variants voted across the wave, without the Cartesian rows where the obstacles
// are out of reach.  Lane m leaves row b 64 + m of the records: stage cost (no terminal term), verdict bits (the rate verdict
// included), (s_N, v_N) and a copy of the scenario's tv_sv and enc -- the network kernel takes one row per state and is not
// taught another indexing.  A wave whose scenario is not alive writes NaN (s_N, v_N) and returns: the network launch reads
// nothing this solve did not write, and a NaN value is never looked at.
// Accept: J_m = stage_m - V_m where feasible and finite, the search's butterfly on (J, m), ties to the lowest m; accepted only if
// strictly below cost_out[b].  The wave then lays trial m out again -- value_trial_column, the statements the trials kernel laid
// it out with, every lane the same column --, rolls it with all rows, lane 0 keeps the states in LDS, and x_out[b], u_out[b],
// cost_out[b] leave as whole rows.  alive[b] becomes the acceptance; argmin_out and status_out are never written.
// LDS: the trial columns, plan and direction (value_trials_lds_doubles), the accept kernel the states as well
// (polish_lds_doubles): above 64 KB from N = 63 on, asked for in prepare_emit_kernels.  Two waves per SIMD as the polish has: the
// roll-out's registers are the search unit's (make resource-usage-polish prints both kernels').
__host__ __device__ inline size_t value_trials_lds_doubles(int N) { return (size_t)2 * N * 64 + 4 * N; }
// The plan u_out[b] into u, its gradient into g (non-finite entries 0), g <- d = -g / scale, and trial m into the calling lane's
// column of slot.  Called by every lane of the scenario's wave.
__device__ __forceinline__ void value_trial_column(const KP& P, const Scenario<double>& S, int b, int m, const double* u_out,
                                                   const double* __restrict__ grad, double* slot, double* u, double* g) {
    const int lane = threadIdx.x, N = P.N, n2 = 2 * N;
    for (int i = lane; i < n2; i += 64) {
        u[i] = u_out[(size_t)b * n2 + i];
        const double gi = grad[(size_t)b * n2 + i];
        g[i] = finite_d(gi) ? gi : 0.0;
    }
    __syncthreads();
    // d = -g / scale: the longest trial moves some input by four rate limits
    double ma = 0.0, md = 0.0;
    for (int k = lane; k < N; k += 64) { ma = fmax(ma, fabs(g[k])); md = fmax(md, fabs(g[N + k])); }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ma = fmax(ma, __shfl_xor(ma, off, 64));
        md = fmax(md, __shfl_xor(md, off, 64));
    }
    const bool steer = P.rate_df > 0.0;
    const double scale = (steer ? fmax(ma / (4.0 * P.rate_a), md / (4.0 * P.rate_df)) : ma / (4.0 * P.rate_a)) + 1e-30;
    __syncthreads();                                      // every lane has read g
    for (int i = lane; i < n2; i += 64) g[i] = (i < N || steer) ? -g[i] / scale : 0.0;
    __syncthreads();
    const double alpha = exp2(-(double)m / 3.0);
    double pa = S.a_prev, pd = S.df_prev;
    for (int k = 0; k < N; ++k) {
        pa = clampd(clampd(u[k] + alpha * g[k], pa - P.rate_a, pa + P.rate_a), P.a_min, P.a_max);
        pd = clampd(clampd(u[N + k] + alpha * g[N + k], pd - P.rate_df, pd + P.rate_df), -P.df_max, P.df_max);
        slot[(size_t)k * 64 + lane] = pa;
        slot[(size_t)(N + k) * 64 + lane] = pd;
    }
}
template <bool HI, int NRK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void value_trials_f64_kernel(
        KP P, int B, int first, const double* __restrict__ x0, const double* __restrict__ u_prev, const double* __restrict__ kparams,
        const uint32_t* __restrict__ flags, const double* __restrict__ obs, const double* __restrict__ cinf,
        const double* __restrict__ tv_sv, const double* __restrict__ enc, const int32_t* __restrict__ status_out,
        const double* __restrict__ u_out, double* work) {
    extern __shared__ double value_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const ValuePolishLayout L(B, P.N);
    int32_t* alive = reinterpret_cast<int32_t*>(work + L.alive());
    const bool live = first ? status_out[b] == 0 : alive[b] != 0;
    if (first && lane == 0) alive[b] = live ? 1 : 0;
    const size_t row = (size_t)b * VALUE_POLISH_TRIALS + lane;
    double2* sv = reinterpret_cast<double2*>(work + L.sv());
    reinterpret_cast<double2*>(work + L.tv_sv())[row] = make_double2(tv_sv[(size_t)b * 2], tv_sv[(size_t)b * 2 + 1]);
    reinterpret_cast<double2*>(work + L.enc())[row] = make_double2(enc[(size_t)b * 2], enc[(size_t)b * 2 + 1]);
    double* stage = work + L.stage();
    uint32_t* feas = reinterpret_cast<uint32_t*>(work + L.feas());
    if (!live) {                                          // unsolved or stopped: defined words, nothing else
        stage[row] = (double)NAN;
        feas[row] = VIOL_NONFINITE;
        sv[row] = make_double2((double)NAN, (double)NAN);
        return;
    }
    const int n2 = 2 * P.N;
    double* slot = value_lds;                             // [2 N][64] the lanes' control sequences
    double* u = slot + (size_t)n2 * 64;                   // [2 N] the plan
    double* g = u + n2;                                   // [2 N] gradient, then direction
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs);
    const bool far = !(P.dev & DEV_NO_FAR) && obstacles_out_of_reach<double>(P, S, lane);
    value_trial_column(P, S, b, lane, u_out, work + L.grad(), slot, u, g);
    NullSink none;
    double J, sN, vN;
    unsigned viol;
    if (far) f64::rollout_one<CAND_TABLE, HI, ROLL_POLISH | ROLL_NO_XY, NRK>(P, S, 0, nullptr, cinf, none, J, viol, sN, vN, slot + lane, 64);
    else f64::rollout_one<CAND_TABLE, HI, ROLL_POLISH, NRK>(P, S, 0, nullptr, cinf, none, J, viol, sN, vN, slot + lane, 64);
    stage[row] = J;
    feas[row] = viol;
    sv[row] = make_double2(sN, vN);
}
template <bool HI, int NRK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void value_accept_f64_kernel(
        KP P, int B, const double* __restrict__ x0, const double* __restrict__ u_prev, const double* __restrict__ kparams,
        const uint32_t* __restrict__ flags, const double* __restrict__ obs, const double* __restrict__ cinf,
        double* __restrict__ cost_out, double* __restrict__ x_out, double* u_out, double* work) {
    extern __shared__ double value_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const ValuePolishLayout L(B, P.N);
    int32_t* alive = reinterpret_cast<int32_t*>(work + L.alive());
    if (alive[b] == 0) return;                            // unsolved or stopped: neither read nor written
    const size_t row = (size_t)b * VALUE_POLISH_TRIALS + lane;
    const double Jm = (work + L.stage())[row] - (work + L.V())[row];          // mpc.py:369
    double bestJ = Jm;
    int bestM = (reinterpret_cast<const uint32_t*>(work + L.feas())[row] == 0 && finite_d(Jm)) ? lane : -1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {             // the search's butterfly on (J, m), ties to the lowest m
        const double oJ = __shfl_xor(bestJ, off, 64);
        const int oM = __shfl_xor(bestM, off, 64);
        const bool take = (oM >= 0) && (bestM < 0 || oJ < bestJ || (oJ == bestJ && oM < bestM));
        if (take) { bestJ = oJ; bestM = oM; }
    }
    const bool accepted = bestM >= 0 && bestJ < cost_out[b];      // only when feasible and strictly cheaper
    if (lane == 0) alive[b] = accepted ? 1 : 0;
    if (!accepted) return;
    const int N = P.N, n2 = 2 * N, nx = 7 * (N + 1);
    double* slot = value_lds;
    double* u = slot + (size_t)n2 * 64;
    double* g = u + n2;
    double* xl = g + n2;                                  // [7][N + 1] the accepted plan's states
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs);
    value_trial_column(P, S, b, bestM, u_out, work + L.grad(), slot, u, g);
    // the accepted trial with all rows: every lane rolls it (one wave's time either way), lane 0 keeps the states
    StoreSink<double> keep{lane == 0 ? xl : nullptr, nullptr, N};
    double J, sN, vN;
    unsigned viol;
    f64::rollout_one<CAND_TABLE, HI, ROLL_POLISH, NRK>(P, S, 0, nullptr, cinf, keep, J, viol, sN, vN, slot + lane, 64);
    __syncthreads();
    for (int i = lane; i < nx; i += 64) x_out[(size_t)b * nx + i] = xl[i];
    for (int i = lane; i < n2; i += 64) u_out[(size_t)b * n2 + i] = slot[(size_t)i * 64 + lane];
    if (lane == 0) cost_out[b] = bestJ;
}

// ---- dJ/du of the progress cost for one control sequence per scenario (igt_cost_gradient_f64) ----
// 64 sequences per wave, one per lane.  Forward sweep: the roll-out of (s, ey, epsi) with the node states kept in LDS,
// [3 (N + 1)][GRAD_STRIDE]; backward sweep: per step the Jacobian at the kept node (igt_adjoint64.h) and the costate update, v
// walked back by v_k = v_k+1 - dt a_k.  The two gradient entries of step k take the slots of node k + 1, which the sweep has just
// left, so at the end the wave's gradients lie in LDS and leave as whole lines: [2 N] doubles per scenario, the 64 scenarios'
// rows contiguous in HBM.  The lane stride is 65 doubles, not 64: the sweeps read a slot across lanes (consecutive words either
// way), the write-out reads one lane's slots (stride 3 x 65 words: spread over the banks; 3 x 64 would put them all on one).
// x, y, psi feed nothing back and are not rolled, so IGT_FLAG_ABS_HEADING (|psi_0|) changes nothing here.  A non-finite cost
// gives a NaN row.  No workspace, no wave votes: lanes past B idle.
// TERM: the terminal term of the cost.  TERM_PROGRESS: -(s_N - s_0) (mpc.py:372), seed (-1, 2 ey_N, 2 epsi_N, 0); vn is not read.
// The value-network cost (igt_cost_gradient_vn_f64, mpc.py:369) runs the kernel twice around terminal_value_f64_kernel, on the
// scratch vn (igt_launch.h VnScratch): TERM_LEAVE is the forward sweep alone and leaves (s_N, v_N); TERM_VALUE reads the network's
// answer for them, J = stage terms - V_out, seed (-dV_out/ds_N, 2 ey_N, 2 epsi_N, -dV_out/dv_N) -- v_N = v_0 + dt sum a_k, so the
// last entry reaches every a_k through costate_step's dt lam[3].
constexpr int GRAD_STRIDE = 65;
enum { TERM_PROGRESS = 0, TERM_LEAVE = 1, TERM_VALUE = 2 };
__host__ __device__ inline size_t grad_lds_doubles(int N) { return (size_t)3 * (N + 1) * GRAD_STRIDE; }
template <int TERM>
__global__ __launch_bounds__(64) void cost_gradient_f64_kernel(KP P, int B, const double* __restrict__ x0,
                                                               const double* __restrict__ kparams, const double* __restrict__ U,
                                                               double* __restrict__ cost_out, double* __restrict__ grad_out,
                                                               double* __restrict__ vn) {
    extern __shared__ double grad_lds[];
    const int lane = threadIdx.x, N = P.N, n2 = 2 * N;
    const int b0 = blockIdx.x * 64, b = b0 + lane;
    if (b < B) {
        adj::StepModel M;
        M.init(P, kparams[(size_t)b * 3 + 0], kparams[(size_t)b * 3 + 1], kparams[(size_t)b * 3 + 2]);
        const double* ua = U + (size_t)b * n2;
        double* node = grad_lds + lane;
        double s = x0[(size_t)b * 7 + 2], ey = x0[(size_t)b * 7 + 3], ep = x0[(size_t)b * 7 + 4], v = x0[(size_t)b * 7 + 5];
        const double s0 = s;
        double J = 0.0, T[3][5];
        node[0] = s; node[GRAD_STRIDE] = ey; node[2 * GRAD_STRIDE] = ep;
        for (int k = 0; k < N; ++k) {
            const double a = ua[k], df = ua[N + k];
            J = J + P.w_u * (a * a + df * df);                                       // mpc.py:362-364
            J = J + ep * ep;
            J = J + ey * ey;
            const adj::Slip sl = adj::slip(M.lr_ratio, df);
            M.step<false>(s, ey, ep, v, a, sl, T);
            v = fma(M.dt, a, v);
            double* nk = node + (size_t)3 * (k + 1) * GRAD_STRIDE;
            nk[0] = s; nk[GRAD_STRIDE] = ey; nk[2 * GRAD_STRIDE] = ep;
        }
        J = J + ep * ep;
        J = J + ey * ey;
        if constexpr (TERM == TERM_LEAVE) {
            double* sv = VnScratch(vn, B).sv();
            sv[(size_t)b * 2 + 0] = s; sv[(size_t)b * 2 + 1] = v;
            return;
        }
        double seed_s = -1.0, seed_v = 0.0;                                          // d (terminal term) / d (s_N, v_N)
        if constexpr (TERM == TERM_VALUE) {
            const VnScratch S(vn, B);
            J = J - S.V()[b];                                                        // mpc.py:369
            seed_s = -S.dV()[(size_t)b * 2 + 0]; seed_v = -S.dV()[(size_t)b * 2 + 1];
        } else {
            J = J - (s - s0);                                                        // mpc.py:372
        }
        cost_out[b] = J;
        double lam[4] = {seed_s, 2.0 * ey, 2.0 * ep, seed_v};
        for (int k = N - 1; k >= 0; --k) {
            const double a = ua[k], df = ua[N + k];
            v = fma(-M.dt, a, v);
            double* nk = node + (size_t)3 * k * GRAD_STRIDE;
            const double sk = nk[0], eyk = nk[GRAD_STRIDE], epk = nk[2 * GRAD_STRIDE];
            adj::step_jacobian(M, sk, eyk, epk, v, a, df, T);
            double ga, gd;
            adj::costate_step(T, M.dt, P.w_u, eyk, epk, a, df, lam, ga, gd);
            nk[3 * GRAD_STRIDE] = ga;                                                // node k + 1's s and ey slots
            nk[4 * GRAD_STRIDE] = gd;
        }
        node[0] = finite_d(J) ? 1.0 : 0.0;                                           // node 0's s slot: the row's verdict
    }
    if constexpr (TERM == TERM_LEAVE) return;
    __syncthreads();
    const int nS = B - b0 < 64 ? B - b0 : 64;
    double* go = grad_out + (size_t)b0 * n2;
    for (int i = lane; i < nS * n2; i += 64) {
        const int sc = i / n2, r = i - sc * n2, row = r >= N ? 1 : 0, k = r - row * N;
        const double gv = grad_lds[(size_t)(3 * (k + 1) + row) * GRAD_STRIDE + sc];
        go[i] = grad_lds[sc] != 0.0 ? gv : (double)NAN;
    }
}

template <int CAND, bool HI, bool OWN = false>      // OWN: `table` is U[B,C,2,N], the scenario rolls its own part of it
__global__ __launch_bounds__(256) void rollout_all_f64_kernel(KP P, int B, const double* __restrict__ x0,
                                                              const double* __restrict__ u_prev,
                                                              const double* __restrict__ kparams,
                                                              const uint32_t* __restrict__ flags,
                                                              const double* __restrict__ obs,
                                                              const double* __restrict__ table,
                                                              const double* __restrict__ cinf, Centre<double> cpar,
                                                              double* __restrict__ X_all, double* __restrict__ U_all,
                                                              double* __restrict__ cost_all, uint32_t* __restrict__ viol_all,
                                                              double* __restrict__ rec_sN, double* __restrict__ rec_vN,
                                                              double* __restrict__ rec_J, uint32_t* __restrict__ rec_viol) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
    for (int c = lane; c < P.C; c += 64) {          // C is a multiple of 64: the wave stays whole (votes inside)
        const size_t bc = (size_t)b * P.C + c;
        StoreSink<double> sink{X_all ? X_all + bc * 7 * (P.N + 1) : nullptr, U_all ? U_all + bc * 2 * P.N : nullptr, P.N};
        double J, sN, vN;
        unsigned viol;
        f64::rollout_one<CAND, HI, ROLL_ALL>(P, S, c, scenario_table(P, table, b, OWN), cinf, sink, J, viol, sN, vN);
        if (rec_J) {   // value-net cost: value_kernel adds the terminal term and fills cost_all / viol_all
            rec_sN[bc] = sN; rec_vN[bc] = vN; rec_J[bc] = J; rec_viol[bc] = viol;
            continue;
        }
        const double Jq = J - (sN - S.x0[2]);
        if (!finite_d(Jq)) viol |= VIOL_NONFINITE;
        cost_all[bc] = Jq;
        viol_all[bc] = viol;
    }
}

// igt_rollout_batch_box_f64: rollout_all_f64_kernel with the rectangle verdict.  One wave per scenario (its table of poses is
// the wave's, in LDS), `obs` the poses [B,n_obs,3,N+1].
template <int CAND, bool HI>
__global__ __launch_bounds__(64) void rollout_all_box_f64_kernel(KP P, int B, const double* __restrict__ x0,
                                                                 const double* __restrict__ u_prev,
                                                                 const double* __restrict__ kparams,
                                                                 const uint32_t* __restrict__ flags,
                                                                 const double* __restrict__ obs,
                                                                 const double* __restrict__ table,
                                                                 const double* __restrict__ cinf, Centre<double> cpar,
                                                                 BoxModel box, double* __restrict__ X_all,
                                                                 double* __restrict__ U_all, double* __restrict__ cost_all,
                                                                 uint32_t* __restrict__ viol_all, double* __restrict__ rec_sN,
                                                                 double* __restrict__ rec_vN, double* __restrict__ rec_J,
                                                                 uint32_t* __restrict__ rec_viol) {
    __shared__ double boxtab[BOX_TAB_DOUBLES];
    const int b = blockIdx.x;
    if (b >= B) return;
    const int lane = threadIdx.x;
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
    f64::fill_box_table(P, box, obs + (size_t)b * P.n_obs * 3 * (P.N + 1), lane, boxtab);
    S.obs = boxtab;
    for (int c = lane; c < P.C; c += 64) {          // C is a multiple of 64: the wave stays whole (votes inside)
        const size_t bc = (size_t)b * P.C + c;
        StoreSink<double> sink{X_all ? X_all + bc * 7 * (P.N + 1) : nullptr, U_all ? U_all + bc * 2 * P.N : nullptr, P.N};
        double J, sN, vN;
        unsigned viol;
        f64::rollout_one<CAND, HI, ROLL_ALL | ROLL_BOX>(P, S, c, table, cinf, sink, J, viol, sN, vN);
        if (rec_J) {   // value-net cost: value_kernel adds the terminal term and fills cost_all / viol_all
            rec_sN[bc] = sN; rec_vN[bc] = vN; rec_J[bc] = J; rec_viol[bc] = viol;
            continue;
        }
        const double Jq = J - (sN - S.x0[2]);
        if (!finite_d(Jq)) viol |= VIOL_NONFINITE;
        cost_all[bc] = Jq;
        viol_all[bc] = viol;
    }
}

#if IGT_DEV_KERNELS
// ---------------------------------------------------------------------------------------
// The LITERAL mapping of BASELINE.json's north_star, kept as a measurement variant (IGT_DEV_FLAGS = 2048):
// one wavefront per (scenario, candidate) trajectory -- lane 0 rolls the horizon (the recurrence is sequential) and
// stages the states in LDS; then the wave evaluates the stage costs and verdicts stage-parallel (lane k = stage k,
// terminal-set facets spread over all 64 lanes), butterfly-reduces them, and the 16 waves of the scenario's workgroup
// take the arg-min over the candidates.  DESIGN.md section 3 has the numbers: the roll-out is 63/64 idle, so this is
// ~40x slower than one lane per candidate; it is NOT a production path (sum order differs from the oracle's).
// ---------------------------------------------------------------------------------------
struct LdsSink {
    static constexpr bool kKeepsStates = true;
    double* x;   // [7, N+1]
    double* u;   // [2, N]
    int N;
    __device__ __forceinline__ void ctrl(int, int k, double a, double df) { u[k] = a; u[N + k] = df; }
    __device__ __forceinline__ void slip(int, int, double, double) {}
    __device__ __forceinline__ void state(int, int k, const double (&st)[7]) {
#pragma unroll
        for (int i = 0; i < 7; ++i) x[i * (N + 1) + k] = st[i];
    }
};
constexpr int LIT_WAVES = 16;      // LIT_MAX_N: igt_launch.h
template <int CAND, bool HI>
__global__ __launch_bounds__(64 * LIT_WAVES) void search_literal_f64_kernel(
    KP P, int B, int W, const double* __restrict__ x0, const double* __restrict__ u_prev, const double* __restrict__ kparams,
    const uint32_t* __restrict__ flags, const double* __restrict__ obs, const double* __restrict__ table,
    const double* __restrict__ cinf, Centre<double> cpar, double* __restrict__ part_J, int32_t* __restrict__ part_c) {
    __shared__ double lds[LIT_WAVES][9 * (LIT_MAX_N + 1)];
    __shared__ double wJ[LIT_WAVES];
    __shared__ int wC[LIT_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    Scenario<double> S;
    load_scenario<double>(S, P, b, x0, u_prev, kparams, flags, obs, cpar);
    double* X = lds[wave];
    double* U = X + 7 * (P.N + 1);
    double bestJ = 0.0;
    int bestC = -1;
    for (int c = wave; c < P.C; c += LIT_WAVES) {
        if (lane == 0) {                       // the trajectory: one lane, the other 63 wait
            LdsSink sink{X, U, P.N};
            double J, sN, vN;
            unsigned viol;
            f64::rollout_one<CAND, HI, ROLL_LITERAL>(P, S, c, table, cinf, sink, J, viol, sN, vN);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        // stage-parallel cost (mpc.py:361-364) and verdicts (mpc.py:296-299, 316-317, 223-226): lane k = stage k
        double part = 0.0, g = -1.0e300;
        for (int k = lane; k <= P.N; k += 64) {
            const double ey = X[3 * (P.N + 1) + k], ep = X[4 * (P.N + 1) + k], v = X[5 * (P.N + 1) + k];
            part += ep * ep + ey * ey;
            g = fmax(g, fabs(ey) - P.ey_lim);
            if (k < P.N) {
                const double a = U[k], df = U[P.N + k];
                part += P.w_u * (a * a + df * df);
                g = fmax(g, fmax(P.v_min - v, v - P.v_max));
            }
            if (k >= 1)
                for (int o = 0; o < P.n_obs; ++o) {
                    const double dx = X[k] - S.obs[(o * 2 + 0) * (P.N + 1) + k], dy = X[(P.N + 1) + k] - S.obs[(o * 2 + 1) * (P.N + 1) + k];
                    g = fmax(g, P.dmin2 - (dx * dx + dy * dy));
                }
        }
        {   // terminal set (mpc.py:177-180): the facets over the lanes
            const double vt = X[5 * (P.N + 1) + P.N - 1], at = U[P.N - 1];
            for (int m = lane; m < P.F; m += 64) g = fmax(g, cinf[m * 3 + 0] * vt + cinf[m * 3 + 1] * at - cinf[m * 3 + 2]);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            part += __shfl_xor(part, off, 64);
            g = fmax(g, __shfl_xor(g, off, 64));
        }
        const double Jq = part - (X[2 * (P.N + 1) + P.N] - S.x0[2]);          // mpc.py:372
        if (g <= P.tol && finite_d(Jq) && (bestC < 0 || Jq < bestJ)) { bestJ = Jq; bestC = c; }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) { wJ[wave] = bestJ; wC[wave] = bestC; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double J = 0.0;
        int c = -1;
        for (int w = 0; w < LIT_WAVES; ++w)
            if (wC[w] >= 0 && (c < 0 || wJ[w] < J || (wJ[w] == J && wC[w] < c))) { J = wJ[w]; c = wC[w]; }
        part_J[(size_t)b * W] = J; part_c[(size_t)b * W] = c;
        for (int w = 1; w < W; ++w) part_c[(size_t)b * W + w] = -1;
    }
}

#endif  // IGT_DEV_KERNELS

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
#if IGT_DEV_KERNELS
template <bool VALUE>
static hipError_t launch_search_exact(const KP& P, int B, const SolveArgs<double>& A, hipStream_t st) {
    typedef ExactStepper<double> St;
    const dim3 grid(A.plan.grid), block(256);
    with_bool(P.cand_mode != CAND_TABLE, [&](auto shared_df) {
        hipLaunchKernelGGL((search_kernel<St, double, 1, shared_df(), VALUE>), grid, block, 0, st, P, B, A.x0, A.u_prev,
                           A.kparams, A.flags, A.obs, A.table, A.cinf, A.centre(), A.cost_out, A.argmin_out, A.status_out,
                           A.rec_sN, A.rec_vN, A.rec_J, A.rec_viol);
    });
    return hipGetLastError();
}

#endif
// The arguments every float64 search kernel takes (IGT_SEARCH64_ARGS), out of SolveArgs; more: what one kernel takes behind
// them (search_f64_kernel_cap: the trajectories)
template <class Kernel, class... More>
static hipError_t launch_search_kernel(Kernel kernel, size_t grid, const KP& Pr, int B, int W, int queues, const unsigned* order,
                                       int order_stride, const SolveArgs<double>& A, hipStream_t st, More... more) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, st, Pr, B, W, queues, A.work_counter, order, order_stride, A.x0, A.u_prev,
                       A.kparams, A.flags, A.obs, A.table, A.cinf, A.centre(), A.part_J, A.part_c, A.rec_sN, A.rec_vN, A.rec_J,
                       A.rec_viol, A.rec_count, A.rec_b, A.unit_seg, more...);
    return hipGetLastError();
}
// f(CAND, HI, NRK) as constants: the candidate family and the build of the control step that P asks for (igt_dispatch.h)
template <class F>
static hipError_t with_build(const KP& P, F&& f) {
    return with_cand(P.cand_mode, [&](auto cand) {
        return with_discretisation(P.hi_order, P.n_rk4, [&](auto hi, auto nrk) { return f(cand, hi, nrk); });
    });
}

// float64 search: the prelude and the kernel that A.plan names (igt_launch.h plan_search64, where the rules and their
// measurements are) -- persistent waves on the per-XCD queues, one 64-candidate unit, or one scenario's pool, at a time
template <int CAND, bool HI, int NRK, bool VALUE>
static hipError_t launch_search64(const KP& P, int B, const SolveArgs<double>& A, hipStream_t st) {
    const Search64Plan& plan = A.plan;
    const int W = plan.W;
    const bool pools = plan.search_kernel == SearchKernel64::POOL;
    KP Pr = P;
    Pr.dev |= plan.launch_dev_bits;      // what the kernel finds behind the partials (PartJTail)
    if constexpr (CAND != CAND_TABLE) {
        if (plan.live_rows) {
            const int n_groups = rows_groups(B, plan.rows_threads, P.G);
            const auto rows = [&](auto threads) {
                with_bool(plan.rows_build_queues, [&](auto queues) {
                    hipLaunchKernelGGL((accel_rows_kernel<CAND, queues(), threads()>), dim3(n_groups + (queues() ? 8 : 0)), dim3(threads()),
                                       0, st, P, B, A.x0, A.u_prev, A.flags, A.cinf, A.centre(), A.row_mask, A.row_rems, W, A.kparams,
                                       A.queue_order, plan.order_stride, A.work_counter, pools ? W : 0);
                });
            };
            if (plan.rows_threads == ROWS_THREADS_NARROW) rows(std::integral_constant<int, ROWS_THREADS_NARROW>{});
            else rows(std::integral_constant<int, ROWS_THREADS_WIDE>{});
        }
    }
    if (plan.separate_queue_builder)
        hipLaunchKernelGGL(build_queues_kernel<double>, dim3(8), dim3(QB_THREADS), 0, st, P, B, W, A.x0, A.kparams, A.queue_order,
                           plan.order_stride, A.work_counter, plan.live_rows ? A.row_mask : nullptr);
    const unsigned* order = plan.sorts_queues() ? A.queue_order : nullptr;
    const auto search = [&](auto kernel, auto... more) {
        return launch_search_kernel(kernel, plan.grid, Pr, B, W, plan.queues, order, plan.order_stride, A, st, more...);
    };
    if (plan.box) {      // the rectangle collision model (plan_box64): A.obs is the poses, A.box the model
        if (plan.search_kernel != SearchKernel64::UNITS || plan.queues != 0 || !(A.box.h0 > 0.0)) return hipErrorInvalidValue;
        return search(search_box_f64_kernel<CAND, HI, VALUE>, A.box);
    }
    switch (plan.search_kernel) {
    case SearchKernel64::CAPTURE_STATIC:
    case SearchKernel64::CAPTURE_QUEUES:
        return search(search_f64_kernel_cap<CAND, VALUE>, A.traj);
    case SearchKernel64::POOL:
        // with checkpoint records to leave (emit in pieces) the build that carries the slots; else the one without them
        if constexpr (CAND == CAND_LATTICE && !VALUE)
            return with_bool((plan.launch_dev_bits & DEV_LAUNCH_CKPT) != 0,
                             [&](auto ckpt) { return search(search_f64_kernel_pool<CAND, HI, VALUE, NRK, ckpt()>); });
        break;
    case SearchKernel64::CANDIDATES_STAGED:      // per-scenario candidate sets (plan_candidates64): A.table is U[B,C,2,N]
        if constexpr (CAND == CAND_TABLE && !VALUE) {
            if (A.table_stride != cand_table_doubles(P.C, P.N) || cand_slab_doubles(P.N) > (size_t)CAND_STAGE_ROWS * 64) break;
            hipLaunchKernelGGL((search_cand_staged_f64_kernel<HI, NRK>), dim3(plan.grid), dim3(64), 0, st, P, B, W, A.x0, A.u_prev, A.kparams,
                               A.flags, A.obs, A.table, A.cinf, A.part_J, A.part_c);
            return hipGetLastError();
        }
        break;
    case SearchKernel64::CANDIDATES_DIRECT:
        if constexpr (CAND == CAND_TABLE) {
            if (A.table_stride != cand_table_doubles(P.C, P.N)) break;
            return search(search_cand_direct_f64_kernel<HI, VALUE, NRK>);
        }
        break;
    case SearchKernel64::UNITS:
        // NRK = 4: the reference's discretisation (4 sub-steps, short polynomials) has its own build of the kernel
        if constexpr (CAND == CAND_TRACK) return search(search_f64_kernel_o2w<CAND, HI, VALUE, NRK>);
        else return search(search_f64_kernel_o2<CAND, HI, VALUE, NRK>);
#if IGT_DEV_KERNELS
    case SearchKernel64::UNITS_WAVES3:
        return search(search_f64_kernel_o3<CAND, HI, VALUE>);
    case SearchKernel64::LITERAL:
        hipLaunchKernelGGL((search_literal_f64_kernel<CAND, HI>), dim3(plan.grid), dim3(64 * LIT_WAVES), 0, st, P, B, W, A.x0, A.u_prev,
                           A.kparams, A.flags, A.obs, A.table, A.cinf, A.centre(), A.part_J, A.part_c);
        return hipGetLastError();
#endif
    default:
        break;
    }
    return hipErrorInvalidValue;      // a plan made for another family, cost or library
}
template <bool VALUE>
static hipError_t dispatch_search64(const KP& P, int B, const SolveArgs<double>& A, hipStream_t st) {
#if IGT_DEV_KERNELS
    if (A.plan.search_kernel == SearchKernel64::ORACLE) return launch_search_exact<VALUE>(P, B, A, st);     // developer switch
#endif
    return with_build(P, [&](auto cand, auto hi, auto nrk) { return launch_search64<cand(), hi(), nrk(), VALUE>(P, B, A, st); });
}
template <>
hipError_t launch_search<double>(const KP& P, int B, const SolveArgs<double>& A, hipStream_t st) {
    return dispatch_search64<false>(P, B, A, st);
}
template <>
hipError_t launch_search_records<double>(const KP& P, int B, const SolveArgs<double>& A, hipStream_t st) {
    return dispatch_search64<true>(P, B, A, st);
}

// emit: the kernel that A.plan names -- the same plan as the search pass's, which left the trajectories or the records it reads
template <int CAND, bool HI, int NRK>
static hipError_t launch_emit64(const KP& P, int B, int W, const SolveArgs<double>& A, hipStream_t st) {
    switch (A.plan.emit_kernel) {
    case EmitKernel64::GATHER:
        hipLaunchKernelGGL((emit_gather_f64_kernel<CAND>), dim3(B), dim3(64), 0, st, P, B, W, A.x0, A.u_prev, A.flags, A.centre(), A.part_J, A.part_c,
                           A.traj,
                           A.cost_out,
                           A.argmin_out, A.status_out, A.x_out, A.u_out);
        break;
    case EmitKernel64::PIECES: {
        const int S = A.plan.seg_scenarios;
        hipLaunchKernelGGL((emit_seg_f64_kernel<CAND, HI, NRK>), dim3((B + S - 1) / S), dim3(SEG_THREADS), A.plan.seg_lds_bytes, st, P,
                           B, W, S, A.x0, A.u_prev, A.kparams, A.flags, A.obs, A.table, A.cinf, A.centre(), A.part_J, A.part_c,
                           A.ck_records, A.cost_out, A.argmin_out, A.status_out, A.x_out, A.u_out);
        break;
    }
    case EmitKernel64::ONE_PIECE: {
        const auto emit = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((B + 63) / 64), dim3(64), 0, st, P, B, W, A.x0, A.u_prev, A.kparams, A.flags, A.obs, A.table,
                               A.cinf, A.centre(), A.part_J, A.part_c, A.cost_out, A.argmin_out, A.status_out, A.x_out, A.u_out);
        };
        // the build that raises its wave priority: asked for behind the pool search alone (plan_search64 emit_priority), so the
        // lattice's emit alone has it.  No per-kernel setup depends on the build (prepare_emit_kernels: emit in pieces and polish).
        if (A.table_stride != 0) {      // per-scenario candidate sets: the scenario's own table
            if constexpr (CAND == CAND_TABLE)
                if (A.table_stride == cand_table_doubles(P.C, P.N) && A.plan.emit_priority == 0) { emit(emit_f64_kernel<CAND, HI, NRK, 0, true>); break; }
            return hipErrorInvalidValue;
        }
        if (A.plan.emit_priority == 0) { emit(emit_f64_kernel<CAND, HI, NRK>); break; }
        if constexpr (CAND == CAND_LATTICE)
            if (A.plan.emit_priority == EMIT_PRIORITY_OVERLAP) { emit(emit_f64_kernel<CAND, HI, NRK, EMIT_PRIORITY_OVERLAP>); break; }
        return hipErrorInvalidValue;      // a plan made for another family or library
    }
    case EmitKernel64::ORACLE:      // launch_emit<double> has taken it
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template <class K>
static hipError_t seg_lds_opt_in(K kernel) {      // once per instantiation and device (a function attribute)
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEG_LDS_MAX);
}
// dynamic LDS above 64 KB has to be asked for, per kernel and device: once per handle at igt_create -- not on the launch path,
// which must stay a pure sequence of stream operations (stream capture).  The emit in pieces and the polish kernel: every build
// the launchers can reach, from the lists they dispatch on.
hipError_t prepare_emit_kernels() {
    hipError_t e = hipSuccess;
    const auto opt_in = [&](auto kernel) { if (e == hipSuccess) e = seg_lds_opt_in(kernel); };
    for_each_discretisation([&](auto hi, auto nrk) {
        for_each_family([&](auto cand) { opt_in(emit_seg_f64_kernel<cand(), hi(), nrk()>); });
        opt_in(polish_f64_kernel<hi(), nrk(), false>);
        opt_in(polish_f64_kernel<hi(), nrk(), true>);
        opt_in(polish_f64_kernel<hi(), nrk(), true, true>);
        opt_in(value_trials_f64_kernel<hi(), nrk()>);
        opt_in(value_accept_f64_kernel<hi(), nrk()>);
    });
    opt_in(cost_gradient_f64_kernel<TERM_PROGRESS>);
    opt_in(cost_gradient_f64_kernel<TERM_LEAVE>);
    opt_in(cost_gradient_f64_kernel<TERM_VALUE>);
    return e;
}

template <>
hipError_t launch_emit<double>(const KP& P, int B, int W, const SolveArgs<double>& A, hipStream_t st) {
#if IGT_DEV_KERNELS
    if (A.plan.emit_kernel == EmitKernel64::ORACLE) {     // developer switch: oracle-order kernels (argmin_out is already final there)
        hipLaunchKernelGGL((emit_kernel<ExactStepper<double>, double>), dim3((B + 63) / 64), dim3(64), 0, st, P, B, A.x0,
                           A.u_prev, A.kparams, A.flags, A.obs, A.table, A.cinf, A.centre(), A.argmin_out, A.x_out, A.u_out);
        return hipGetLastError();
    }
#endif
    return with_build(P, [&](auto cand, auto hi, auto nrk) { return launch_emit64<cand(), hi(), nrk()>(P, B, W, A, st); });
}

// polish_iters > 0: after emit, on the same stream (igt_api.hip solve_impl).  The kernel's LDS passes 64 KB from N = 63 on: it is
// asked for once per handle (prepare_emit_kernels), like the emit in pieces'.
// adjoint: the gradient of every iteration is the analytic one (igt_set_polish_gradient); the same grid, block and LDS.
// newton: the Newton build (igt_set_polish_step), analytic gradient whatever `adjoint` says; its LDS is 2 N doubles larger.
hipError_t launch_polish(const KP& P, int B, int iters, bool adjoint, bool newton, const SolveArgs<double>& A, hipStream_t st) {
    if (P.dev & (DEV_EXACT64 | DEV_LITERAL)) return hipErrorNotSupported;      // the oracle-order developer kernels
    if (newton) {
        const size_t lds = polish_newton_lds_doubles(P.N) * 8;
        return with_discretisation(P.hi_order, P.n_rk4, [&](auto hi, auto nrk) {
            hipLaunchKernelGGL((polish_f64_kernel<hi(), nrk(), true, true>), dim3(B), dim3(64), lds, st, P, B, iters, A.x0, A.u_prev,
                               A.kparams, A.flags, A.obs, A.cinf, A.status_out, A.cost_out, A.x_out, A.u_out);
            return hipGetLastError();
        });
    }
    const size_t lds = polish_lds_doubles(P.N) * 8;
    return with_discretisation(P.hi_order, P.n_rk4, [&](auto hi, auto nrk) {
        return with_bool(adjoint, [&](auto adj) {
            hipLaunchKernelGGL((polish_f64_kernel<hi(), nrk(), adj()>), dim3(B), dim3(64), lds, st, P, B, iters, A.x0, A.u_prev,
                               A.kparams, A.flags, A.obs, A.cinf, A.status_out, A.cost_out, A.x_out, A.u_out);
            return hipGetLastError();
        });
    });
}

// igt_set_value_polish: launches 4 and 6 of an iteration (see value_trials_f64_kernel); grids of B, nothing read back
hipError_t launch_value_trials(const KP& P, int B, bool first, const SolveArgs<double>& A, double* work, hipStream_t st) {
    if (P.dev & (DEV_EXACT64 | DEV_LITERAL)) return hipErrorNotSupported;      // the oracle-order developer kernels
    const size_t lds = value_trials_lds_doubles(P.N) * 8;
    return with_discretisation(P.hi_order, P.n_rk4, [&](auto hi, auto nrk) {
        hipLaunchKernelGGL((value_trials_f64_kernel<hi(), nrk()>), dim3(B), dim3(64), lds, st, P, B, first ? 1 : 0, A.x0, A.u_prev,
                           A.kparams, A.flags, A.obs, A.cinf, A.tv_sv, A.enc, A.status_out, A.u_out, work);
        return hipGetLastError();
    });
}
hipError_t launch_value_accept(const KP& P, int B, const SolveArgs<double>& A, double* work, hipStream_t st) {
    if (P.dev & (DEV_EXACT64 | DEV_LITERAL)) return hipErrorNotSupported;
    const size_t lds = polish_lds_doubles(P.N) * 8;
    return with_discretisation(P.hi_order, P.n_rk4, [&](auto hi, auto nrk) {
        hipLaunchKernelGGL((value_accept_f64_kernel<hi(), nrk()>), dim3(B), dim3(64), lds, st, P, B, A.x0, A.u_prev, A.kparams,
                           A.flags, A.obs, A.cinf, A.cost_out, A.x_out, A.u_out, work);
        return hipGetLastError();
    });
}

// igt_cost_gradient_f64: one wave per 64 scenarios; the LDS passes 64 KB from N = 41 on (asked for in prepare_emit_kernels)
hipError_t launch_cost_gradient(const KP& P, int B, const double* x0, const double* kparams, const double* U, double* cost_out,
                                double* grad_out, hipStream_t st) {
    hipLaunchKernelGGL(cost_gradient_f64_kernel<TERM_PROGRESS>, dim3((B + 63) / 64), dim3(64), grad_lds_doubles(P.N) * 8, st, P, B,
                       x0, kparams, U, cost_out, grad_out, (double*)nullptr);
    return hipGetLastError();
}
// igt_cost_gradient_vn_f64: the sweeps before (leave = true: (s_N, v_N) into vn) and behind launch_terminal_value
hipError_t launch_cost_gradient_vn(const KP& P, int B, bool leave, const double* x0, const double* kparams, const double* U,
                                   double* cost_out, double* grad_out, double* vn, hipStream_t st) {
    const dim3 grid((B + 63) / 64), block(64);
    const size_t lds = grad_lds_doubles(P.N) * 8;
    if (leave) hipLaunchKernelGGL(cost_gradient_f64_kernel<TERM_LEAVE>, grid, block, lds, st, P, B, x0, kparams, U, cost_out, grad_out, vn);
    else hipLaunchKernelGGL(cost_gradient_f64_kernel<TERM_VALUE>, grid, block, lds, st, P, B, x0, kparams, U, cost_out, grad_out, vn);
    return hipGetLastError();
}

template <>
hipError_t launch_rollout_all<double>(const KP& P, int B, const SolveArgs<double>& A, double* X_all, double* U_all,
                                      double* cost_all, uint32_t* viol_all, hipStream_t st) {
    // the arguments every roll-out of every candidate takes; model: what the rectangle kernel takes between them (A.box)
    const auto launch = [&](auto kernel, dim3 grid, dim3 block, auto... model) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, P, B, A.x0, A.u_prev, A.kparams, A.flags, A.obs, A.table, A.cinf, A.centre(),
                           model..., X_all, U_all, cost_all, viol_all, A.rec_sN, A.rec_vN, A.rec_J, A.rec_viol);
        return hipGetLastError();
    };
    const dim3 grid4((B + 3) / 4), block4(256);      // four scenarios per workgroup, a wave each
#if IGT_DEV_KERNELS
    if (P.dev & DEV_EXACT64)      // developer switch: oracle-order kernels
        return launch(rollout_all_kernel<ExactStepper<double>, double>, grid4, block4);
#endif
    if (A.box.h0 > 0.0) {           // the rectangle collision model: A.obs is the poses [B,n_obs,3,N+1]
        if (A.table_stride != 0) return hipErrorInvalidValue;
        return with_family(P.cand_mode, P.hi_order, [&](auto cand, auto hi) {
            return launch(rollout_all_box_f64_kernel<cand(), hi()>, dim3(B), dim3(64), A.box);
        });
    }
    if (A.table_stride != 0) {      // per-scenario candidate sets: A.table is U[B,C,2,N]
        if (P.cand_mode != CAND_TABLE || A.table_stride != cand_table_doubles(P.C, P.N)) return hipErrorInvalidValue;
        return with_bool(P.hi_order != 0, [&](auto hi) {
            return launch(rollout_all_f64_kernel<CAND_TABLE, hi(), true>, grid4, block4);
        });
    }
    return with_family(P.cand_mode, P.hi_order, [&](auto cand, auto hi) {
        return launch(rollout_all_f64_kernel<cand(), hi()>, grid4, block4);
    });
}

}  // namespace igt
