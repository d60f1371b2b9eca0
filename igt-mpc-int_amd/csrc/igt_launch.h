// igt_launch.h -- launcher declarations shared by igt_kernels.hip and igt_api.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <type_traits>
#include "igt_device.h"
#include "igt_value_net.h"
#include "igt_value_polish_layout.h"

namespace igt {

// trajectories kept by the search pass of a small double batch (igt_kernels_common.h CaptureSink)
constexpr int TRAJ_FIELDS = 9;                    // the 7 states, then a and delta_f
__host__ __device__ inline size_t traj_unit_doubles(int N) { return (size_t)TRAJ_FIELDS * (N + 1) * 64; }
constexpr int CK_RECORD_DOUBLES = 24;             // igt_fast64.h (CK_PARTS - 1) * CK_FIELDS
constexpr int QB_THREADS = 1024, QB_TRIPS = 2;    // build_queues_kernel: up to 2048 units per queue (B <= 8192 at W = 2)
constexpr int LIT_MAX_N = 40;                     // search_literal_f64_kernel's LDS holds horizons up to this
// emit_seg_f64_kernel stages this much per scenario in LDS; scenarios per workgroup: a full wave's 64 when their staging fits a
// compute unit's LDS (116 KB at N = 20; 160 KB per CU, the kernel asks for more than the default 64 KB: seg_lds_opt_in), else
// the largest power of two that does
__host__ __device__ inline int seg_doubles_per_scenario(int N) { return 7 * (N + 1) + 4 * N; }
constexpr size_t SEG_LDS_MAX = 150 * 1024;
inline int seg_scenarios_per_block(int N) {
    int S = 64;
    while (S > 0 && (size_t)S * seg_doubles_per_scenario(N) * 8 > SEG_LDS_MAX) S >>= 1;
    return S;
}

// ---- the grid of the persistent float64 search (plan_search64) ----
// The wave slots a search may take: two waves per SIMD (three: the developer builds of DEV_WAVES3), or one where the caller has
// announced three or more solves in flight (Search64Env::waves_per_simd == 1), so that two searches are resident side by side.
// The pools' batch bound (B >= 4 * slots) is stated in these, reserve or not: which kernel runs does not depend on the reserve.
inline size_t search64_slots(int n_cu, int waves_per_simd, int dev, bool dev_kernels = IGT_DEV_KERNELS) {
    const bool o3 = dev_kernels && (dev & DEV_WAVES3) != 0;
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
inline size_t search64_grid(int n_cu, int waves_per_simd, Search64 family, int dev, int reserve_per_8cu = -1,
                            bool dev_kernels = IGT_DEV_KERNELS) {
    const size_t slots = search64_slots(n_cu, waves_per_simd, dev, dev_kernels);
    if (waves_per_simd != 1 || (dev & DEV_NO_RESERVE) || (dev_kernels && (dev & DEV_WAVES3))) return slots;
    const int per8 = reserve_per_8cu >= 0 ? reserve_per_8cu
                                          : (family == Search64::POOL ? SEARCH64_RESERVE_PER_8CU_POOL : SEARCH64_RESERVE_PER_8CU_UNITS);
    const size_t reserve = (size_t)n_cu * (size_t)per8 / 8;
    const size_t floor = slots < (size_t)SEARCH64_QUEUES ? slots : (size_t)SEARCH64_QUEUES;
    return slots > reserve + floor ? slots - reserve : floor;
}

// ---- the workgroups of the acceleration-row pass (igt_kernels_f64.hip accel_rows_kernel) ----
// One lane per (scenario, row), 64 / G scenarios per wave; workgroups of ROWS_THREADS_WIDE threads, or -- plan_search64
// rows_threads -- of one wave.  What the launcher and the kernel both count with:
constexpr int ROWS_THREADS_WIDE = 256, ROWS_THREADS_NARROW = 64;
inline int rows_scenarios_per_block(int threads, int G) { return (threads / 64) * (64 / G); }
inline int rows_groups(int B, int threads, int G) {      // row workgroups (the queue builders come on top)
    const int per_block = rows_scenarios_per_block(threads, G);
    return (B + per_block - 1) / per_block;
}

// ---- the plan of one float64 solve: what it runs, decided once on the host ----
// plan_search64 states the search kernel, its prelude, the launch-time bits, the emit kernel, the workspace and the counter memset.
// igt_api.hip solve_impl carves its workspace from the plan; launch_search64 / launch_emit64 (igt_kernels_f64.hip) switch on it.
// Host code over KP and plain numbers, no pointers: tests/search_plan.cpp checks it without a GPU.
enum class SearchKernel64 {
    ORACLE,           // search_kernel<ExactStepper>: the oracle-order developer kernel (DEV_EXACT64)
    LITERAL,          // search_literal_f64_kernel: the literal wave-per-trajectory mapping (DEV_LITERAL), a measurement variant
    CAPTURE_STATIC,   // search_f64_kernel_cap, one wave per unit: no queues, no counters
    CAPTURE_QUEUES,   // search_f64_kernel_cap on the queues
    POOL,             // search_f64_kernel_pool: one item per scenario
    UNITS_WAVES3,     // search_f64_kernel_o3: the 3-waves-per-SIMD developer builds (DEV_WAVES3)
    UNITS,            // search_f64_kernel_o2 / _o2w (tracking family) on 64-candidate units
    // per-scenario candidate sets U[B,C,2,N] (plan_candidates64; never chosen by plan_search64)
    CANDIDATES_STAGED,   // search_cand_staged_f64_kernel: the unit's slab of U staged in LDS, one wave per unit
    CANDIDATES_DIRECT,   // search_cand_direct_f64_kernel: search_unit64 on the scenario's own table, one wave per unit
};
enum class EmitKernel64 {
    ORACLE,           // emit_kernel<ExactStepper>
    GATHER,           // emit_gather_f64_kernel: copies the winner out of the trajectories the search kept
    PIECES,           // emit_seg_f64_kernel: rolls the winner in four pieces from the search's checkpoint records
    ONE_PIECE,        // emit_f64_kernel
};
struct Search64Env {      // what the plan reads besides KP, the batch size and the cost
    int n_cu;
    int waves_per_simd;   // of the persistent search grid: 2, or 1 when solves overlap (igt_set_concurrency >= 3)
    int reserve_pool = -1, reserve_units = -1;   // developer sweeps: search64_grid's reserve_per_8cu by kernel family (-1: the shipped values)
    int dev_traj_max = -1;                       // developer sweeps (IGT_DEV_TRAJ_MAX): the batch size up to which trajectories are kept
    bool dev_kernels = IGT_DEV_KERNELS;          // the library carries the developer kernels; without them igt_create refuses their flags
};
constexpr int EMIT_PRIORITY_OVERLAP = 3;         // s_setprio level of the one-piece emit beside resident searches (plan_search64 emit_priority)
struct Search64Plan {
    int W;                            // 64-candidate units per scenario
    int partials;                     // [B, partials] part_J / part_c: one per unit
    SearchKernel64 search_kernel;
    size_t grid;                      // workgroups of the search kernel
    int queues;                       // 8, or 0: every unit has a wave of its own
    int order_stride;                 // entries per queue of the unit order (the pools' items are scenarios)
    bool live_rows;                   // accel_rows_kernel runs: units of live acceleration rows only
    bool rows_build_queues;           // ... and sorts the queues in the same launch
    int rows_threads = ROWS_THREADS_WIDE;   // ... in workgroups of this many threads: ROWS_THREADS_WIDE, or ROWS_THREADS_NARROW when solves overlap
    bool separate_queue_builder;      // build_queues_kernel runs
    int launch_dev_bits;              // OR-ed into the search kernel's KP::dev (DEV_LAUNCH_CKPT, DEV_LAUNCH_LIVE_ROWS)
    EmitKernel64 emit_kernel;
    int seg_scenarios;                // PIECES: scenarios per workgroup ...
    size_t seg_lds_bytes;             // ... and their dynamic LDS
    // workspace to carve; 0: not taken.  Trajectories and queue order exactly where the chosen kernels touch them.
    size_t traj_doubles;              // [B W][9][N+1][64] trajectories (the capture kinds -> GATHER)
    size_t ck_records;                // [B W] checkpoint records of CK_RECORD_DOUBLES behind the partials (PIECES reads them)
    size_t queue_order_words;         // [8][ceil(B/8) W] unit order of the queues (either queue builder)
    bool memset_counters;             // the host zeroes the unit counters: queues that no builder zeroes
    bool reset_rec_count;             // value-network cost: the host zeroes rec_count before every pass (the compact list's lengths)
    int emit_priority;                // ONE_PIECE: the wave priority emit_f64_kernel sets at its top (0: none)
    bool box = false;                 // plan_box64 alone: the UNITS are search_box_f64_kernel's -- the rectangle verdict, a plain grid
    bool sorts_queues() const { return rows_build_queues || separate_queue_builder; }
    // what only a float solve has (Search32Plan): solve_impl reads either plan under one set of names
    static constexpr size_t ckpt_doubles = 0;
    static constexpr bool reset_best_key = false;
};

// value: the pass writes per-candidate records for the value network (launch_search_records), else the progress cost.
// P.refine_it is not read: one plan serves every refinement pass of a solve.
inline Search64Plan plan_search64(const KP& P, int B, bool value, const Search64Env& env) {
    Search64Plan p{};
    const int W = p.W = p.partials = P.C / 64;
    const size_t total = (size_t)B * W;
    p.order_stride = ((B + 7) / 8) * W;
    if (env.dev_kernels && (P.dev & DEV_EXACT64)) {      // developer switch: oracle-order kernels, four scenarios per workgroup
        p.search_kernel = SearchKernel64::ORACLE;
        p.emit_kernel = EmitKernel64::ORACLE;
        p.grid = ((size_t)B + 3) / 4;
        return p;
    }
    if (env.dev_kernels && (P.dev & DEV_LITERAL) && !value && P.N <= LIT_MAX_N) {
        p.search_kernel = SearchKernel64::LITERAL;
        p.emit_kernel = EmitKernel64::ONE_PIECE;
        p.grid = (size_t)B;
        return p;
    }
    // 2 waves per SIMD (232 VGPRs, no spill); the 3-per-SIMD build spills 244 B/lane and is 3-8 % behind at every batch
    // size (DEV_WAVES3 selects it for A/B runs)
    const bool o3 = env.dev_kernels && (P.dev & DEV_WAVES3) != 0;

    // Small batches -- no more units than the chip has SIMDs, B <= 256 at 256 candidates -- keep the trajectories of the search
    // pass and emit copies the winner's (igt_kernels_common.h CaptureSink; 97 KB of stores per unit at N = 20, hidden behind a
    // lone wave's dependent chains; with several units per SIMD they are not: a closed loop of 512 problems per step ran 0.32 ms
    // per step with them against 0.30 without, 0.43 against 0.36 at 1024), when the kernel built for the reference's
    // discretisation runs; DEV_NO_CAPTURE switches it off for A/B runs.
    const size_t traj_max_units = env.dev_traj_max >= 0 ? (size_t)(env.dev_traj_max < 8192 ? env.dev_traj_max : 8192) * W   // sweeps: a batch size
                                                        : (size_t)env.n_cu * 4;
    const bool captures_trajectories = total <= traj_max_units && P.C % 64 == 0 && !P.hi_order && P.n_rk4 == 4 &&
                                       !(P.dev & (DEV_WAVES3 | DEV_EXACT64 | DEV_LITERAL | DEV_NO_CAPTURE));
    // ... and such a batch has no more units than the chip has SIMDs (the kernel that keeps trajectories holds one wave per
    // SIMD), so every unit is given its own wave: the queue builder (6.6 us and a launch) would only order units that all start
    // at once.  Measured, search + emit, tracking family: 67 us against 84 at B = 1, 91 against 101 at B = 32.
    // DEV_KEEP_QUEUES keeps the queues for A/B runs; the unit trace (DEV_TRACE) needs them.
    const bool search_is_static = captures_trajectories && total <= (size_t)env.n_cu * 4 && !(P.dev & (DEV_TRACE | DEV_KEEP_QUEUES));

    // Small batches: the search queues are sorted longest unit first (build_queues_kernel, or inside accel_rows_kernel; 3-5 % up
    // to B = 4096, nothing from 8192 on); the builder also zeroes the unit counters.
    const bool search_builds_queues = !search_is_static && B <= 6144 && W <= 256 && ((B + 7) / 8) * W <= QB_THREADS * QB_TRIPS &&
                                      !(P.dev & (DEV_NO_QUEUE_ORDER | DEV_EXACT64 | DEV_LITERAL));

    // Emit rolls the winner in four pieces from the search pass's checkpoints (emit_seg_f64_kernel): progress cost (with the
    // value network the winner is only known after the network has run), batches that do not keep trajectories, horizons of at
    // least 8 steps.  Not when the caller overlaps solves (igt_set_concurrency >= 3): there the emit pass of one solve runs under
    // the search pass of another, its latency is hidden, and what matters is that it gets on the chip between two persistent
    // search kernels -- one 64-thread wave without LDS does, a 320-thread workgroup with 116 KB of LDS waits for a compute unit
    // to drain (measured on one box, three runs each: 20.3 against 20.9 M solves/s with four solves in flight).
    const int S = seg_scenarios_per_block(P.N);
    const bool emits_in_pieces = !value && P.N >= 8 && !captures_trajectories && S >= 4 && env.waves_per_simd != 1 &&
                                 !(P.dev & (DEV_WAVES3 | DEV_EXACT64 | DEV_LITERAL | DEV_NO_SEG_EMIT));

    // The search runs on units made of live acceleration rows only (accel_rows_kernel; unit_layout).  Only for batches of more
    // than two rounds of units (B > 1024 at 256 candidates): below that the solve lasts as long as its longest unit, fewer units
    // do not shorten it, and the extra launch costs 8 us (a closed loop of 512 problems per step: 0.30 against 0.28 ms).
    const bool packs_live_rows = P.cand_mode != CAND_TABLE && P.G <= 64 && P.G * P.G == P.C && W * 64 == P.C && P.G % W == 0 &&
                                 !(P.dev & (DEV_NO_SLICES | DEV_EXACT64 | DEV_LITERAL | DEV_ALL_ROWS)) && !captures_trajectories &&
                                 total > (size_t)env.n_cu * 16;

    // Lattice on live rows: one item per scenario, its candidates rolled as one pool by a wave whose lanes refill (search_pool64):
    // progress cost, the steering table of all G columns fits.  Every developer switch that changes the units' layout keeps the
    // units (the A/B comparisons of the units stay what they were), and so does DEV_NO_REFILL; so do the queues sorted by
    // build_queues_kernel (DEV_SEPARATE_QUEUES), which knows only units.
    // An item is about four units long, and with fewer than four per wave the longest items make the span (one solve at a time,
    // B = 4096: 2 per wave, search 0.208 -> 0.230 ms; four solves in flight, one wave per SIMD: 4 per wave, 23.6 -> 27.0 M solves/s).
    // The slots bound the pools' batch; the waves launched leave a reserve when solves overlap (search64_grid).
    const bool search_pools = !o3 && P.cand_mode == CAND_LATTICE && !value && packs_live_rows &&
                              P.G * P.N <= STEER_TABLE_MAX_ENTRIES &&
                              !(P.dev & (DEV_NO_SLICES | DEV_NO_EARLY_EXIT | DEV_NO_STEER_TABLE | DEV_ALL_ROWS | DEV_WHOLE_COLUMNS |
                                         DEV_NO_REFILL | DEV_SEPARATE_QUEUES | DEV_WAVES3)) &&
                              (size_t)B >= 4 * search64_slots(env.n_cu, env.waves_per_simd, P.dev, env.dev_kernels);

    p.search_kernel = search_is_static        ? SearchKernel64::CAPTURE_STATIC
                      : captures_trajectories ? SearchKernel64::CAPTURE_QUEUES
                      : search_pools          ? SearchKernel64::POOL
                      : o3                    ? SearchKernel64::UNITS_WAVES3
                                              : SearchKernel64::UNITS;
    p.emit_kernel = captures_trajectories ? EmitKernel64::GATHER : emits_in_pieces ? EmitKernel64::PIECES : EmitKernel64::ONE_PIECE;
    if (search_is_static) {
        p.grid = total;
    } else {
        const size_t items = search_pools ? (size_t)B : total;
        const size_t waves = search64_grid(env.n_cu, env.waves_per_simd, search_pools ? Search64::POOL : Search64::UNITS, P.dev,
                                           search_pools ? env.reserve_pool : env.reserve_units, env.dev_kernels);
        p.grid = items < waves ? items : waves;
        p.queues = SEARCH64_QUEUES;
    }
    if (search_pools) p.order_stride = (B + 7) / 8;
    p.live_rows = packs_live_rows;
    p.rows_build_queues = packs_live_rows && search_builds_queues && !(P.dev & DEV_SEPARATE_QUEUES);
    p.separate_queue_builder = search_builds_queues && !p.rows_build_queues;
    // Solves that overlap (igt_set_concurrency >= 3): the row pass runs beside two resident searches that hold nearly every wave
    // slot, and a workgroup starts only where ONE compute unit has all its waves' slots free at once.  One-wave workgroups: row
    // pass 106 -> 50 us under overlap, headline +7.3 % with the builder's empty trips gone, tracking family +6.2 %
    // (profiles/rows_shape_ab.txt); DEV_WIDE_ROWS keeps the 256 threads for A/B runs.
    p.rows_threads = packs_live_rows && env.waves_per_simd == 1 && !(P.dev & DEV_WIDE_ROWS) ? ROWS_THREADS_NARROW : ROWS_THREADS_WIDE;
    // The one-piece emit of overlapping solves: one wave per 64 scenarios, each a single dependent chain of some 27 000
    // instructions, and always the youngest wave on a SIMD that holds one or two persistent search waves -- VALU issue goes by
    // priority, then age, so it gets the slots the searches leave: 49 us alone on the chip, 162 us beside them.  Behind the pool
    // search the wave raises its priority once at its top (s_setprio, never lowered; emit_f64_kernel PRIO): the chain issues
    // every few cycles at the most, the searches keep the rest, the work done is the same.
    // Measured (profiles/rows_in_search_ab.txt; five alternating runs a side): headline 34.75 -> 35.77 M solves/s
    // (+2.9 %, every run above every parent run, parent spread 0.33 %), three in flight 30.51 -> 34.39 (+12.7 %); emit under
    // overlap 160 -> 109 us, pool search 269 -> 285, row pass 50 -> 80 (sum 480 -> 474).  Levels 1, 2 and 3 gave one figure --
    // the searches stay at 0 -- so it is 3.  Pool search only: the tracking family's emit fell as well (281 -> 267 us) but its
    // unit search paid more than that, -0.9 % on the step, so the 64-candidate units keep priority 0 and only the lattice's
    // emit has the raised build.
    // DEV_EMIT_PRIO0 keeps priority 0 for A/B runs.
    p.emit_priority = search_pools && p.emit_kernel == EmitKernel64::ONE_PIECE && env.waves_per_simd == 1 && !(P.dev & DEV_EMIT_PRIO0)
                          ? EMIT_PRIORITY_OVERLAP : 0;
    // the live-row masks and the checkpoint records live behind the partials (PartJTail): no further kernel argument -- the
    // search kernels spill scalar registers as it is, and every one more shows up as v_readlane in the control-step loop
    p.launch_dev_bits = (emits_in_pieces ? DEV_LAUNCH_CKPT : 0) | (packs_live_rows ? DEV_LAUNCH_LIVE_ROWS : 0);
    if (emits_in_pieces) {
        p.seg_scenarios = S;
        p.seg_lds_bytes = (size_t)S * seg_doubles_per_scenario(P.N) * 8;
    }
    // The records are taken for every progress-cost solve of 8 steps or more, also where emit rolls in one piece and nothing
    // touches them: behind the partials they set where part_c, the unit counters and the queue order lie, and without their
    // 3 MB the headline (B = 4096, four solves in flight, emit in one piece) ran 0.1294 against 0.1272 ms per step, same device
    // code (profiles/search_plan_identity.txt, section 4).
    if (!value && P.N >= 8) p.ck_records = total;
    if (captures_trajectories) p.traj_doubles = total * traj_unit_doubles(P.N);
    if (search_builds_queues) p.queue_order_words = (size_t)((B + 7) / 8) * 8 * W;
    p.memset_counters = !search_is_static && !search_builds_queues;
    p.reset_rec_count = value;
    return p;
}

// ---- the plan of a solve on per-scenario candidate sets U[B,C,2,N] (igt_solve_candidates_f64) ----
// The table family with a table of the scenario's own.  Every other input of the solve together is 1.8 MB at B = 4096; U is
// 335 MB at C = 256, N = 20, and no two units read the same bytes: a streaming read with a roll-out behind it.
//   * progress cost, the unit's slab U[b, 64 p .. 64 p + 63, :, :] -- 2 N 64 contiguous doubles -- fits an eighth of a compute
//     unit's LDS (N <= 20: 20 KB, eight waves a compute unit, the two per SIMD the roll-out's registers allow):
//     CANDIDATES_STAGED loads it once and rolls from LDS;
//   * longer horizons, and the value-network cost (whose units leave records, not partials): CANDIDATES_DIRECT, search_unit64
//     on the scenario's table in HBM.
// A plain grid of one wave per unit, no queues, no counters, no prelude.  Nothing keeps trajectories or checkpoint records, so
// emit rolls the winner in one piece at every batch size (at priority 0) and the workspace is the partials alone.
constexpr size_t CAND_LDS_BUDGET = 160 * 1024, CAND_SLAB_MAX_BYTES = CAND_LDS_BUDGET / 8;
__host__ __device__ inline size_t cand_table_doubles(int C, int N) { return (size_t)C * 2 * N; }      // one scenario's U[b]
__host__ __device__ inline size_t cand_slab_doubles(int N) { return (size_t)2 * N * 64; }              // one unit's part of it
inline Search64Plan plan_candidates64(const KP& P, int B, bool value) {
    Search64Plan p{};
    p.W = p.partials = P.C / 64;
    p.grid = (size_t)B * p.W;
    p.order_stride = ((B + 7) / 8) * p.W;
    const bool staged = !value && cand_slab_doubles(P.N) * 8 <= CAND_SLAB_MAX_BYTES;
    p.search_kernel = staged ? SearchKernel64::CANDIDATES_STAGED : SearchKernel64::CANDIDATES_DIRECT;
    p.emit_kernel = EmitKernel64::ONE_PIECE;
    p.reset_rec_count = value;
    return p;      // queues 0, no prelude, no launch-time bits, no trajectories, records or queue order, no counter memset, priority 0
}

// ---- the plan of a solve under the rectangle (OBCA) collision model (igt_solve_batch_box_f64) ----
// Any candidate family, either cost.  search_box_f64_kernel on a plain grid of one wave per (scenario, 64-candidate unit): no
// queues, no counters, no prelude (every acceleration row is rolled), no launch-time bits.  Nothing keeps trajectories or
// checkpoint records, so emit rolls the winner in one piece at every batch size (at priority 0; it judges nothing, so it is
// the circle entries' kernel) and the workspace is the partials alone.
inline Search64Plan plan_box64(const KP& P, int B, bool value) {
    Search64Plan p{};
    p.W = p.partials = P.C / 64;
    p.grid = (size_t)B * p.W;
    p.order_stride = ((B + 7) / 8) * p.W;
    p.search_kernel = SearchKernel64::UNITS;      // 64-candidate units ...
    p.box = true;                                 // ... of search_box_f64_kernel, one wave each: queues 0
    p.emit_kernel = EmitKernel64::ONE_PIECE;
    p.reset_rec_count = value;
    return p;
}
// The model a kernel takes (igt_device.h BoxModel) from the entry's three scalars -> nullptr, or what the entries refuse the
// values with (non-finite or non-positive extents; d_box non-finite or negative), nothing written: the one place that judges
// them.  1e-6: the reference's margin on the distance (mpc.py:221).
inline const char* box_model(double length, double width, double d_box, BoxModel* out) {
    const auto finite = [](double v) { return v - v == 0.0; };
    if (!finite(length) || !(length > 0.0)) return "box collision model: length must be finite and positive";
    if (!finite(width) || !(width > 0.0)) return "box collision model: width must be finite and positive";
    if (!finite(d_box) || !(d_box >= 0.0)) return "box collision model: d_box must be finite and not below 0";
    BoxModel m;
    m.h0 = 0.5 * length; m.h1 = 0.5 * width; m.dsafe = d_box + 1e-6;
    const double rho = std::sqrt(m.h0 * m.h0 + m.h1 * m.h1), gate = m.dsafe + 2.0 * rho;
    m.gate2 = gate * gate;
    *out = m;
    return nullptr;
}

// ---- the plan of one float solve: what it runs, decided once on the host ----
// plan_search32 states the search kernel and its grid, the queue builder, the tracking family's incumbents, the checkpoints and
// the emit kernel, the workspace and the memsets.  igt_api.hip solve_impl carves its workspace from the plan; launch_search_fast /
// launch_emit_fast (igt_kernels.hip) switch on it.  Host code over KP and plain numbers, no pointers: tests/search_plan32.cpp
// checks it without a GPU.
enum class SearchKernel32 {
    WAVES3,           // search_fast_kernel_o3: the 3-waves-per-SIMD developer builds (DEV_WAVES3)
    CHECKPOINTS,      // search_fast_kernel_o2c: leaves horizon checkpoints for the emit in pieces
    TRACK,            // search_fast_kernel_o2w: the tracking family, held to two waves per SIMD
    UNITS,            // search_fast_kernel_o2
};
enum class EmitKernel32 {
    PIECES,           // emit_seg_kernel: ck_parts lanes per scenario roll the winner's pieces from the search's checkpoints
    ONE_PIECE,        // emit_fast_kernel
};
struct Search32Env {      // what the plan reads besides KP, the batch size and the cost
    int n_cu;
    int waves_per_simd;   // of the persistent search grid: 2, or 1 when solves overlap (igt_set_concurrency >= 3)
    int dev_ckpt = -1;                           // developer sweeps (IGT_DEV_CKPT): the pieces of the emit (-1, 0: the shipped rule)
    bool dev_kernels = IGT_DEV_KERNELS;          // the library carries the developer kernels; without them igt_create refuses their flags
};
constexpr int SEARCH32_QUEUES = 8;
struct Search32Plan {
    int W;                            // units per scenario: 128-candidate slices, two candidates per lane
    int partials;                     // [B, partials] part_J / part_c: one per unit, or one per scenario (value-network cost)
    SearchKernel32 search_kernel;
    size_t grid;                      // workgroups (one wave each) of the search kernel
    int queues;                       // SEARCH32_QUEUES, always
    int order_stride;                 // entries per queue of the unit order
    bool builds_queues;               // build_queues_kernel<float> runs: the queues longest unit first, the unit counters zeroed
    int launch_dev_bits;              // OR-ed into the search kernel's and the builder's KP::dev (DEV_LAUNCH_INCUMBENTS)
    int ck_parts;                     // pieces the horizon is emitted in (igt_device.h Seg / Ckpt): 1, 2, 4 -- up to SEG_MAX_PARTS
    EmitKernel32 emit_kernel;
    size_t emit_grid;                 // workgroups (one wave each) of the emit kernel
    // workspace to carve; 0: not taken
    size_t ckpt_doubles;              // [ck_parts - 1][B W][SEG_UNIT_DOUBLES] horizon checkpoints of the search pass for emit
    size_t queue_order_words;         // [8][ceil(B/8) W] unit order of the queues
    bool memset_counters;             // the host zeroes the unit counters: no builder does
    bool reset_rec_count, reset_best_key;   // value-network cost: the host resets the compact list's length (0) and the [B] keys (0xff)
    // the [B] incumbents behind the partials are in use: the host sets them to "none" (0xff) before every pass
    bool incumbents() const { return (launch_dev_bits & DEV_LAUNCH_INCUMBENTS) != 0; }
    // what only a float64 solve has (Search64Plan): solve_impl reads either plan under one set of names
    static constexpr size_t ck_records = 0, traj_doubles = 0;
};

// value: the pass appends the feasible candidates to the compact list for the value network (launch_search_records), else the
// progress cost.  P.refine_it is not read: one plan serves every refinement pass of a solve.
inline Search32Plan plan_search32(const KP& P, int B, bool value, const Search32Env& env) {
    Search32Plan p{};
    // units per scenario of the search kernel: 128-candidate slices (two candidates per lane; an odd number of 64-candidate
    // chunks: the last slice rolls its chunk twice)
    const int W = p.W = (P.C + 127) / 128;
    // per-scenario partials: the value path reduces to ONE per scenario (compact list + atomicMin), the progress cost keeps
    // one per 128-candidate slice
    p.partials = value ? 1 : W;
    const size_t total = (size_t)B * W;
    // persistent waves on per-XCD queues, 2 per SIMD.  The 3-per-SIMD build (168 VGPRs, a spill around each unit) was
    // ahead on big batches in round 1; with the sub-step variants unrolled it spills 228 B/lane and is behind at every
    // size but one (B = 32 768: +0.7 %) -- it stays selectable for A/B runs (DEV_WAVES3)
    const bool o3 = env.dev_kernels && (P.dev & DEV_WAVES3) != 0;
    const size_t slots = (size_t)env.n_cu * 4 * (o3 ? 3 : (env.waves_per_simd == 1 ? 1 : 2));
    p.grid = total < slots ? total : slots;
    p.queues = SEARCH32_QUEUES;
    p.order_stride = ((B + 7) / 8) * W;

    // small float batches: emit in 4 pieces from checkpoints of the search pass.  Measured (search + emit): +15 % at
    // B = 1024, +12 % at 2048, +3 % at 4096, -1 % at 8192 -- but the records are ~150 MB of HBM writes per B = 4096 solve
    // against ~1 MB of algorithmic traffic, so they are only spent where emit latency dominates.
    int ck_parts = 1;
    if (B <= 2048 && P.N % 4 == 0 && P.N >= 8) ck_parts = 4;
    else if (B <= 2048 && P.N % 2 == 0 && P.N >= 4) ck_parts = 2;
    if (env.dev_ckpt >= 1 && env.dev_ckpt <= SEG_MAX_PARTS && P.N % env.dev_ckpt == 0 && P.N >= 2 * env.dev_ckpt)
        ck_parts = env.dev_ckpt;      // threshold sweeps, at every batch size; a count the horizon does not take is ignored
    // The 3-per-SIMD build leaves no checkpoints, so its solves emit in one piece.  (Before the plan the search launcher took
    // the _o3 build first and the emit launcher the checkpoints all the same: a DEV_WAVES3 solve of B <= 2048 emitted its
    // pieces from checkpoints nobody had written.  No test ran one; tests/search_plan32.cpp states both sides.)
    if (o3) ck_parts = 1;
    p.ck_parts = ck_parts;
    const bool ckpt = ck_parts > 1;
    if (ckpt) p.ckpt_doubles = (size_t)(ck_parts - 1) * total * SEG_UNIT_DOUBLES;

    // Small batches: the search queues are sorted longest unit first (build_queues_kernel), which also zeroes the unit counters.
    // The order words are taken for every B <= 6144, also where no builder runs (W > 256, a queue longer than the builder's
    // QB_THREADS * QB_TRIPS, DEV_NO_QUEUE_ORDER): they lie in front of the value path's records, and on the float64 side moving
    // one such array changed the headline by 2 % with identical kernels (profiles/search_plan_identity.txt, section 4) -- the
    // workspace stays where it was measured.
    if (B <= 6144) p.queue_order_words = (size_t)((B + 7) / 8) * 8 * W;
    p.builds_queues = p.queue_order_words != 0 && W <= 256 && ((B + 7) / 8) * W <= QB_THREADS * QB_TRIPS && !(P.dev & DEV_NO_QUEUE_ORDER);
    p.memset_counters = !p.builds_queues;

    // tracking family, progress cost: units of acceleration rows (igt_kernels.hip accel_units), pruned against the scenario's
    // incumbent (igt_fast64.h BOUND).  The [B] keys behind the partials start every pass at "none" (all ones: above every
    // cost's key).  Not with one unit per scenario -- nothing to prune against -- and not with DEV_NO_BOUND.
    if (P.cand_mode == CAND_TRACK && !value && P.G * P.G == P.C && W * 128 == P.C && P.G >= 16 && P.G <= 64 &&
        !(P.dev & (DEV_NO_SLICES | DEV_STEER_SLICES | DEV_NO_BOUND)) && W > 1)
        p.launch_dev_bits |= DEV_LAUNCH_INCUMBENTS;

    p.search_kernel = o3                          ? SearchKernel32::WAVES3
                      : ckpt                      ? SearchKernel32::CHECKPOINTS
                      : P.cand_mode == CAND_TRACK ? SearchKernel32::TRACK
                                                  : SearchKernel32::UNITS;
    // emit: ck_parts lanes per scenario on the checkpoints, else one lane per scenario
    p.emit_kernel = ckpt ? EmitKernel32::PIECES : EmitKernel32::ONE_PIECE;
    p.emit_grid = ((size_t)B * ck_parts + 63) / 64;
    p.reset_rec_count = p.reset_best_key = value;
    return p;
}

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
    size_t table_stride = 0;   // doubles from one scenario's table to the next: 0, one table shared by the batch (every entry
                               // but the two on per-scenario candidate sets); cand_table_doubles(C, N), table is U[B,C,2,N]
    const double* cinf;   // [F,3] or null
    const double* cpar;    // [B,4] ramp-hold centre offset / span of a refinement pass, or null (first pass)
    const T* u_ws;         // [B,2,N] warm start (previous solution shifted by one step), or null; used where flags & 2
    BoxModel box{};        // h0 > 0 (the _box entries, double): obs is the poses [B,n_obs,3,N+1] and collisions are the rectangles'
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
    int n_cu;                       // compute units: the grids of the value-network kernels (launch_value)
    // what the search and emit launchers run, and what solve_impl carved for them (plan_search32; plan_search64 / plan_candidates64)
    std::conditional_t<sizeof(T) == 4, Search32Plan, Search64Plan> plan;
    double* ckpt;                   // float path: [ck_parts-1][B W] horizon checkpoints of the search pass for emit (null: none)
    unsigned* queue_order;          // [8][ceil(B/8) W] longest-first unit order of the search queues (null: not taken)
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

template <typename T> hipError_t launch_search(const KP& P, int B, const SolveArgs<T>& A, hipStream_t st);
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
// igt_forecast_batch_pose_f64 / igt_forecast_scene_pose_f64: the two forecasts with a heading row behind x, y (obs_pose[..,3,N+1]);
// heads[n_routes,3] = (h0, hN, abs) of igt_set_route_headings.  float64 only: the box solve that reads a pose has no float entry.
hipError_t launch_forecast_pose(const KP& P, int B, const double* routes, int n_routes, const double* heads,
                                const double* ego_xyh, const double* opp, const double* opp_a, const int32_t* opp_route,
                                const double* opp_heading, const double* plan_x, const double* plan_u, const int32_t* has_plan,
                                double* obs_pose, double* tv_sv, hipStream_t st);
hipError_t launch_forecast_scene_pose(const KP& P, int E, const double* routes, int n_routes, const double* heads,
                                      const double* x, const double* a_prev, const int32_t* route, const double* plan_x,
                                      const double* plan_u, const int32_t* has_plan, double* obs_pose, double* tv_sv,
                                      hipStream_t st);
// ---- igt_loop_advance_*: the closed-loop step behind a solve (igt_kernels.hip loop_advance_kernel) ----
// A workgroup of LOOP_THREADS lanes owns LOOP_AGENTS consecutive agents.  Its lanes 0 .. agents - 1 decide and step one agent each;
// then all of its lanes walk the agents' rows of x_sol and of u_sol -- contiguous per agent, so one contiguous span per
// workgroup -- with consecutive lanes on consecutive elements.  What the launcher, the kernel and tests/loop_advance_shape.cpp
// count with:
constexpr int LOOP_THREADS = 256, LOOP_AGENTS = 16;
inline int loop_grid(int n) { return (int)(((size_t)(n > 0 ? n : 0) + LOOP_AGENTS - 1) / LOOP_AGENTS); }
__host__ __device__ inline int loop_block_agents(int n, int block) {      // agents of workgroup `block`: LOOP_AGENTS, fewer in the last
    const long long left = (long long)n - (long long)block * LOOP_AGENTS;
    return left >= LOOP_AGENTS ? LOOP_AGENTS : (left > 0 ? (int)left : 0);
}
// lane `thread`'s elements of a span of `agents` rows of `row` elements each: f(offset into the span)
template <class F>
__host__ __device__ inline void loop_walk(int agents, size_t row, int thread, F&& f) {
    const size_t span = (size_t)agents * row;
    for (size_t e = (size_t)thread; e < span; e += LOOP_THREADS) f(e);
}
// The buffers of one call.  x / u_prev are read from *_in and written to *_out: one array in device mode, the staged input and
// output copies in host mode (a lane reads its agent's row before it writes it).
template <typename T>
struct LoopArgs {
    const double* x_in; double* x_out;                  // [n,7]
    const double* u_in; double* u_out;                  // [n,2]
    const double* kparams;                              // [n,3]
    const int32_t* status;                              // [n]
    const T *x_sol, *u_sol;                             // [n,7,N+1], [n,2,N]
    double a_brake;
    int32_t* has_plan;                                  // [n]
    T *plan_x, *plan_u, *u_ws;                          // u_ws may be null
    const uint32_t* flags_in; uint32_t* flags_out;      // both or neither null
    int64_t* infeasible;                                // may be null
    double *x_log, *u_log; const int64_t* step; int32_t T_log;      // logs: both or neither null
};
template <typename T> hipError_t launch_loop_advance(const KP& P, int n, const LoopArgs<T>& A, hipStream_t st);
template <typename T> hipError_t launch_first_controls(int B, int N, const T* u, T* u0, hipStream_t st);
template <typename T>
hipError_t launch_cartesian(int n, int steps, double dt, double l_r, double l_f, const T* z0, const T* u, T* z_out,
                            hipStream_t st);

}  // namespace igt
