// igt_launch.h -- launcher declarations shared by igt_kernels.hip and igt_api.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "igt_device.h"
#include "igt_value_net.h"
#include "igt_value_polish_layout.h"

namespace igt {

// trajectories kept by the search pass of a small double batch (igt_kernels_common.h CaptureSink)
constexpr int TRAJ_FIELDS = 9;                    // the 7 states, then a and delta_f
__host__ __device__ inline size_t traj_unit_doubles(int N) { return (size_t)TRAJ_FIELDS * (N + 1) * 64; }

template <typename T>
struct SolveArgs {   // all device pointers
    const T* x0;
    const T* u_prev;
    const T* kparams;
    const uint32_t* flags;
    const T* obs;
    const T* tv_sv;
    const T* enc;
    const double* table;   // [C,2,N] or null
    const double* cinf;    // [F,3] or null
    const double* cpar;    // [B,4] ramp-hold centre offset / span of a refinement pass, or null (first pass)
    const T* u_ws;         // [B,2,N] warm start (previous solution shifted by one step), or null; used where flags & 2
    Centre<T> centre() const { return Centre<T>{cpar, u_ws}; }
    T* x_out;
    T* u_out;
    T* cost_out;
    int32_t* argmin_out;
    int32_t* status_out;
    double* part_J;        // [B, W] per-slice best cost        (workspace)
    int32_t* part_c;       // [B, W] per-slice best candidate
    // value-net cost: per-candidate records written by the search pass, consumed by value_kernel
    T* rec_sN;             // [B, C]
    T* rec_vN;             // [B, C]
    double* rec_J;         // [B, C] cost without the terminal term
    uint32_t* rec_viol;    // [B, C]
    T* p_vec;              // [B, 128] first-layer offsets
    // float path: feasible candidates appended by the search pass (count, scenario, candidate in rec_viol's storage)
    unsigned* work_counter;         // the search's 8 unit counters, 256 B apart (zeroed before every launch); unit_trace behind them
    int n_cu;                       // compute units (sizes the persistent search grid)
    int waves_per_simd;             // of the persistent search grid: 2, or 1 when solves overlap (igt_set_concurrency); 0 = 2
    int reserve_pool = -1, reserve_units = -1;   // developer sweeps: search64_grid's reserve_per_8cu by kernel family (-1: the shipped values)
    double* ckpt;                   // [ck_parts-1][B*Wk] horizon checkpoints of the search pass for emit (null: none)
    int ck_parts;                   // pieces the horizon is emitted in (igt_device.h Seg / Ckpt)
    unsigned* queue_order;          // [8][ceil(B/8) W] longest-first unit order of the search queues (null: index order)
    unsigned* rec_count;
    int32_t* rec_b;
    unsigned long long* best_key;   // [B] per-scenario (orderable cost, candidate) minimum
    int2* unit_seg;                 // double path: [B, C/64] (first entry, count) of each unit's entries in the compact list
    double* prune_thr;              // double path: [B] cost above which an entry cannot win (value_bound_kernel)
    unsigned* live_idx;             // double path: entries left for the network after value_prune_kernel
    double* traj;                   // double path, small batches: [B C/64][9][N+1][64] kept by the search pass (null: none)
    // in part_J behind the partials (PartJTail)
    unsigned long long* row_mask;   // double path: [B] live acceleration rows of the generated families (accel_rows_kernel)
    unsigned long long* incumbents; // [B] the tracking family's best cost keys of the pass (igt_fast64.h BOUND)
    double* row_rems;               // double path: [B G] the acceleration rows' travel sums (accel_rows_kernel)
    double* ck_records;             // double path: [B W][CK_RECORD_DOUBLES] unit winners' checkpoints for emit (null: none)
};
constexpr int CK_RECORD_DOUBLES = 24;   // igt_fast64.h (CK_PARTS - 1) * CK_FIELDS

// What part_J holds behind its [B, W] partials:
//   double path: [B] live-row masks, [B] incumbents, [B G] row travel sums, [B W][CK_RECORD_DOUBLES] checkpoint records
//                (the records only where the host takes them: doubles(true));
//   float path:  [B] incumbents.
// The host takes part_J at doubles() and names the pieces in SolveArgs; the search kernels find them from part_J through the
// same declaration, because their argument lists must not grow (launch_search64) -- launch-time bits of KP::dev say which are
// in use.
template <typename T>
struct PartJTail {
    double* part_J;
    size_t B, W, G;
    __host__ __device__ PartJTail(double* part_J_, int B_, int W_, int G_)
        : part_J(part_J_), B((size_t)B_), W((size_t)W_), G((size_t)G_) {}
    __host__ __device__ size_t doubles(bool ck) const {
        return sizeof(T) == 8 ? B * W + 2 * B + B * G + (ck ? B * W * CK_RECORD_DOUBLES : 0) : B * W + B;
    }
    __host__ __device__ unsigned long long* masks() const { return reinterpret_cast<unsigned long long*>(part_J + B * W); }
    __host__ __device__ unsigned long long* incumbents() const {
        return reinterpret_cast<unsigned long long*>(part_J + B * W) + (sizeof(T) == 8 ? B : 0);
    }
    __host__ __device__ double* row_rems() const { return part_J + B * W + 2 * B; }
    __host__ __device__ double* ck_records() const { return part_J + B * W + 2 * B + B * G; }
};

// What igt_cost_gradient_vn_f64 keeps in the workspace between its three launches, per scenario: the terminal ego state the
// forward sweep leaves, [B, 2] (s_N, v_N); the network's scaled value for it, [B]; its partials by (s_N, v_N), [B, 2].  The
// host takes doubles(B) of the workspace, the sweep kernel finds the pieces from the base through the same declaration.
struct VnScratch {
    double* base;
    size_t B;
    __host__ __device__ VnScratch(double* base_, int B_) : base(base_), B((size_t)B_) {}
    __host__ __device__ static size_t doubles(int B_) { return (size_t)VN_DOUBLES_PER_SCENARIO * (size_t)B_; }
    __host__ __device__ double* sv() const { return base; }
    __host__ __device__ double* V() const { return base + 2 * B; }
    __host__ __device__ double* dV() const { return base + 3 * B; }
};

// work_counter is followed by the developer unit trace (DEV_TRACE): u64[queue items][4]
constexpr size_t WORK_COUNTER_WORDS = 1024;
__host__ __device__ inline unsigned long long* unit_trace(unsigned* work_counter) {
    return reinterpret_cast<unsigned long long*>(work_counter + WORK_COUNTER_WORDS);
}

// ---- the grid of the persistent float64 search (launch_search64) ----
// The wave slots a search may take: two waves per SIMD (three: the developer builds of DEV_WAVES3), or one where the caller has
// announced three or more solves in flight (SolveArgs::waves_per_simd == 1), so that two searches are resident side by side.
// The pools' batch bound (B >= 4 * slots) is stated in these, reserve or not: which kernel runs does not depend on the reserve.
inline size_t search64_slots(int n_cu, int waves_per_simd, int dev) {
    const bool o3 = IGT_DEV_KERNELS && (dev & DEV_WAVES3) != 0;
    return (size_t)n_cu * 4 * (o3 ? 3 : (waves_per_simd == 1 ? 1 : 2));
}
// The persistent waves a search launches.  With one wave per SIMD two resident searches take every slot of the chip between
// them (the pool kernel's registers leave room for two waves per SIMD and no third).  From three solves in flight on a search
// leaves `reserve` slots alone.  The waves dequeue their items, so a smaller grid gives each wave more items and nothing else
// changes -- the same answers, bit for bit.  Measured with four solves in flight (profiles/slot_reserve_ab.txt, DESIGN section
// 3): +4 % on the step rate with 32 of 1024 waves held back, less with 64 and 128, nothing with 256 -- though the other lanes'
// emit and row passes, for which the reserve was meant, take as long as before: the search enqueued behind the two resident
// ones takes the free slots and starts its longest items early.  With three in flight it costs 1.3 %.
// reserve = n_cu * (waves per 8 compute units) / 8, by kernel family; the grid never goes below one wave per queue
// (SEARCH64_QUEUES, one per XCD) while the chip has that many slots and never above the slots.  With one or two solves in
// flight, with DEV_NO_RESERVE and for the DEV_WAVES3 builds: the slots.
// reserve_per_8cu >= 0: the developer library's override for sweeps (IGT_DEV_RESERVE, IGT_DEV_RESERVE_UNITS; igt_api.hip).
enum class Search64 { UNITS, POOL };       // search_f64_kernel_o2 / _o2w on 64-candidate units; search_f64_kernel_pool
constexpr int SEARCH64_QUEUES = 8;
constexpr int SEARCH64_RESERVE_PER_8CU_POOL = 1;       // 32 of 1024 waves at 256 compute units: the value that won the headline's sweep
constexpr int SEARCH64_RESERVE_PER_8CU_UNITS = 0;      // the tracking family's gain (+3 %) stayed under three times its spread: the slots
inline size_t search64_grid(int n_cu, int waves_per_simd, Search64 family, int dev, int reserve_per_8cu = -1) {
    const size_t slots = search64_slots(n_cu, waves_per_simd, dev);
    if (waves_per_simd != 1 || (dev & DEV_NO_RESERVE) || (IGT_DEV_KERNELS && (dev & DEV_WAVES3))) return slots;
    const int per8 = reserve_per_8cu >= 0 ? reserve_per_8cu
                                          : (family == Search64::POOL ? SEARCH64_RESERVE_PER_8CU_POOL : SEARCH64_RESERVE_PER_8CU_UNITS);
    const size_t reserve = (size_t)n_cu * (size_t)per8 / 8;
    const size_t floor = slots < (size_t)SEARCH64_QUEUES ? slots : (size_t)SEARCH64_QUEUES;
    return slots > reserve + floor ? slots - reserve : floor;
}

bool search_builds_queues(const KP& P, int B, const SolveArgs<float>& A);   // then no memset of the counters is needed
bool search_builds_queues(const KP& P, int B, const SolveArgs<double>& A);
bool search_is_static(const KP& P, int B, const SolveArgs<double>& A);      // one wave per unit: no queues, no counters
inline bool search_is_static(const KP&, int, const SolveArgs<float>&) { return false; }
template <typename T> hipError_t launch_search(const KP& P, int B, const SolveArgs<T>& A, int nc, hipStream_t st);
template <typename T> hipError_t launch_emit(const KP& P, int B, int W, const SolveArgs<T>& A, hipStream_t st);
// value-net cost: search pass that writes per-candidate records, then prep + MLP + per-chunk arg-min
template <typename T> hipError_t launch_search_records(const KP& P, int B, const SolveArgs<T>& A, hipStream_t st);
template <typename T>
hipError_t launch_value(const KP& P, int B, const DevNet<T>& net, const SolveArgs<T>& A, T* cost_all,
                        uint32_t* viol_all, hipStream_t st);
hipError_t prepare_value_kernels(int n_hidden_mats);   // once per igt_set_value_net: dynamic-LDS function attributes
hipError_t prepare_emit_kernels();                     // once per igt_create: the same for the float64 emit in pieces
// polish_iters > 0 (float64, progress cost): projected-gradient steps on the emitted winners, in place in A's outputs
hipError_t launch_polish(const KP& P, int B, int iters, bool adjoint, bool newton, const SolveArgs<double>& A, hipStream_t st);
hipError_t launch_cost_gradient(const KP& P, int B, const double* x0, const double* kparams, const double* U, double* cost_out,
                                double* grad_out, hipStream_t st);
// igt_cost_gradient_vn_f64: the sweep before (leave: forward only, (s_N, v_N) into vn) and behind launch_terminal_value
hipError_t launch_cost_gradient_vn(const KP& P, int B, bool leave, const double* x0, const double* kparams, const double* U,
                                   double* cost_out, double* grad_out, double* vn, hipStream_t st);
// igt_terminal_value_f64 (igt_value_net.h terminal_value_f64_kernel); dV_out null: the values alone
hipError_t launch_terminal_value(const DevNet<double>& net, int n_cu, int n, const double* sv, const double* tv_sv,
                                 const double* enc, double* V_out, double* dV_out, hipStream_t st);
// igt_set_value_polish (float64, value-network cost): launches 4 and 6 of one iteration on the emitted winners, in place in A's
// outputs; work: the solve's ValuePolishLayout scratch (igt_value_polish_layout.h).  first: alive[b] is status_out[b] == 0.
// Between them the caller runs launch_terminal_value over the 64 B trial records.
hipError_t launch_value_trials(const KP& P, int B, bool first, const SolveArgs<double>& A, double* work, hipStream_t st);
hipError_t launch_value_accept(const KP& P, int B, const SolveArgs<double>& A, double* work, hipStream_t st);
template <typename T> hipError_t launch_reduce(int B, int W, const SolveArgs<T>& A, hipStream_t st);
// ramp-hold refinement: winner of the pass just finished -> centre/span of the next pass (cpar[B,4])
template <typename T>
hipError_t launch_refine(const KP& P, int B, int W, const SolveArgs<T>& A, double* cpar, int first, hipStream_t st);
template <typename T>
hipError_t launch_rollout_all(const KP& P, int B, const SolveArgs<T>& A, T* X_all, T* U_all, T* cost_all,
                              uint32_t* viol_all, hipStream_t st);   // value mode: also fills A.rec_*
template <typename T>
hipError_t launch_frenet_step(const KP& P, int n, const T* x, const T* u, const T* kparams, T* x_next, hipStream_t st);
template <typename T>
hipError_t launch_forecast(const KP& P, int B, const double* routes, int n_routes, const T* ego_xyh, const T* opp,
                           const T* opp_a, const int32_t* opp_route, const T* plan_x, const T* plan_u,
                           const int32_t* has_plan, T* obs_xy, T* tv_sv, hipStream_t st);
// igt_forecast_scene_*: E scenes of n_obs + 1 agents, scene-major inputs, every agent forecast once and filtered per ego
template <typename T>
hipError_t launch_forecast_scene(const KP& P, int E, const double* routes, int n_routes, const T* x, const T* a_prev,
                                 const int32_t* route, const T* plan_x, const T* plan_u, const int32_t* has_plan, T* obs_xy,
                                 T* tv_sv, hipStream_t st);
template <typename T> hipError_t launch_first_controls(int B, int N, const T* u, T* u0, hipStream_t st);
template <typename T>
hipError_t launch_cartesian(int n, int steps, double dt, double l_r, double l_f, const T* z0, const T* u, T* z_out,
                            hipStream_t st);

}  // namespace igt
