// Stand-alone check of the plan of a float64 solve (csrc/igt_launch.h plan_search64; test_search_plan_host.py builds the
// host side of it with the address / undefined-behaviour sanitizers and runs it).
//
// Before the plan, one question was answered in three places: solve_impl carved the workspace (which pointers are null),
// launch_search64 re-derived the kernel from the pointers through six predicates and a sequence of early returns, launch_emit64
// asked two of the predicates again.  This program restates those three places as they were written -- pointers as booleans, the
// predicates under their names, the returns in their order -- and compares every field of the plan with what they did, over
//   the four families x both costs x B in {1, 32, 256, 257, 1024, 1025, 4095, 4096, 6144, 6145, 65536} x C in {64, 256, 1024}
//   x N in {4, 7, 8, 20, 40, 64} x n_rk4 in {2, 4} x hi_order x n_cu in {8, 256, 304} x waves_per_simd in {1, 2}
//   x {no switch, each switch the predicates read alone} x {no override, IGT_DEV_TRAJ_MAX 0 and 600, both reserves}
// and both kinds of library; the switches that select developer kernels (DEV_WAVES3, DEV_EXACT64, DEV_LITERAL) only with the
// library that carries them: igt_create refuses them otherwise.
// One difference is meant: the literal mapping uses no unit counters, the host used to zero them all the same, the plan does not.
// Then what held by convention only: gather <=> the search kept trajectories, pieces <=> DEV_LAUNCH_CKPT, no queues <=> the
// static capture, the memset exactly where queues run that no builder zeroes, trajectories and queue order taken exactly where
// the chosen kernels touch them (the checkpoint records: wherever the parent took them, see check_point), and the grid of every
// kernel on the queues = min(items, search64_grid of its family).
#include "igt_launch.h"

#include <cstdio>
#include <cstdlib>

using namespace igt;

static long n_points = 0;
static KP g_P;
static int g_B, g_value;
static Search64Env g_env;

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::fprintf(stderr, "%s:%d: %s\n  cand %d value %d B %d C %d N %d n_rk4 %d hi %d dev %d n_cu %d wps %d traj_max %d " \
                         "reserves %d %d dev_kernels %d\n", __FILE__, __LINE__, #cond, g_P.cand_mode, g_value, g_B, g_P.C, g_P.N,  \
                         g_P.n_rk4, g_P.hi_order, g_P.dev, g_env.n_cu, g_env.waves_per_simd, g_env.dev_traj_max,                 \
                         g_env.reserve_pool, g_env.reserve_units, (int)g_env.dev_kernels);                                       \
            std::exit(1);                                                                                                        \
        }                                                                                                                        \
    } while (0)

// ---- the parent's three places, restated ----
namespace parent {

struct Args {      // SolveArgs<double>: the pointers the predicates tested, as "not null"; the numbers they read
    bool traj, ck_records, row_mask, queue_order;
    int n_cu, waves_per_simd, reserve_pool, reserve_units;
};
// solve_impl<double>: what it carved
static Args carve(const KP& P, int B, bool value, const Search64Env& env) {
    const size_t Wk = (size_t)P.C / 64;
    const bool exact64 = (P.dev & DEV_EXACT64) != 0;
    size_t traj_max_units = (size_t)env.n_cu * 4;
    if (env.dev_traj_max >= 0) traj_max_units = (size_t)(env.dev_traj_max < 8192 ? env.dev_traj_max : 8192) * Wk;
    Args A{};
    A.traj = !exact64 && (size_t)B * Wk <= traj_max_units && (P.C % 64) == 0;
    A.ck_records = !value && !exact64 && P.N >= 8;
    A.row_mask = true;
    A.queue_order = B <= 6144;
    A.n_cu = env.n_cu; A.waves_per_simd = env.waves_per_simd; A.reserve_pool = env.reserve_pool; A.reserve_units = env.reserve_units;
    return A;
}
static bool search_builds_queues(const KP& P, int B, const Args& A) {
    const int W = P.C / 64;
    return A.queue_order && W <= 256 && ((B + 7) / 8) * W <= 1024 * 2 && !(P.dev & DEV_NO_QUEUE_ORDER) &&
           !(P.dev & (DEV_EXACT64 | DEV_LITERAL));
}
static bool captures_trajectories(const KP& P, const Args& A) {
    return A.traj && !P.hi_order && P.n_rk4 == 4 && !(P.dev & (DEV_WAVES3 | DEV_EXACT64 | DEV_LITERAL | DEV_NO_CAPTURE));
}
static bool search_is_static(const KP& P, int B, const Args& A) {
    return captures_trajectories(P, A) && (size_t)B * (P.C / 64) <= (size_t)A.n_cu * 4 && !(P.dev & (DEV_TRACE | DEV_KEEP_QUEUES));
}
static int seg_scenarios_per_block(const KP& P) {
    int S = 64;
    while (S > 0 && (size_t)S * (7 * (P.N + 1) + 4 * P.N) * 8 > 150 * 1024) S >>= 1;
    return S;
}
static bool emits_in_pieces(const KP& P, const Args& A) {
    return A.ck_records && P.cost_mode == 0 && P.N >= 8 && !captures_trajectories(P, A) && seg_scenarios_per_block(P) >= 4 &&
           A.waves_per_simd != 1 && !(P.dev & (DEV_WAVES3 | DEV_EXACT64 | DEV_LITERAL | DEV_NO_SEG_EMIT));
}
static bool packs_live_rows(const KP& P, int B, const Args& A) {
    const int W = P.C / 64;
    return A.row_mask && P.cand_mode != CAND_TABLE && P.G <= 64 && P.G * P.G == P.C && W * 64 == P.C && P.G % W == 0 &&
           !(P.dev & (DEV_NO_SLICES | DEV_EXACT64 | DEV_LITERAL | DEV_ALL_ROWS)) && !captures_trajectories(P, A) &&
           (size_t)B * W > (size_t)A.n_cu * 16;
}
static bool search_pools(const KP& P, int cand, bool value, bool live_rows) {
    return cand == CAND_LATTICE && !value && live_rows && P.G * P.N <= 360 &&
           !(P.dev & (DEV_NO_SLICES | DEV_NO_EARLY_EXIT | DEV_NO_STEER_TABLE | DEV_ALL_ROWS | DEV_WHOLE_COLUMNS | DEV_NO_REFILL |
                      DEV_SEPARATE_QUEUES | DEV_WAVES3));
}
static size_t slots(int n_cu, int wps, int dev, bool dev_kernels) {
    return (size_t)n_cu * 4 * (dev_kernels && (dev & DEV_WAVES3) ? 3 : (wps == 1 ? 1 : 2));
}
static size_t grid(int n_cu, int wps, bool pool, int dev, int per8_override, bool dev_kernels) {
    const size_t s = slots(n_cu, wps, dev, dev_kernels);
    if (wps != 1 || (dev & DEV_NO_RESERVE) || (dev_kernels && (dev & DEV_WAVES3))) return s;
    const int per8 = per8_override >= 0 ? per8_override : (pool ? 1 : 0);
    const size_t reserve = (size_t)n_cu * (size_t)per8 / 8, floor = s < 8 ? s : 8;
    return s > reserve + floor ? s - reserve : floor;
}

struct Did {      // what the launchers enqueued
    SearchKernel64 search; size_t grid; int queues; bool order; int order_stride; int kernel_dev_bits;
    bool rows_kernel, rows_with_queues, rows_pool_arg, build_queues_kernel, build_queues_rows;
    EmitKernel64 emit; int S; size_t lds;
    bool memset;
};
// dispatch_search64 + launch_search64<CAND, HI, NRK, VALUE>, return by return
static void search(const KP& P, int B, bool VALUE, const Args& A, bool dev_kernels, Did& d) {
    const int CAND = P.cand_mode;
    const bool HI = P.hi_order != 0;
    const int W = P.C / 64;
    if (dev_kernels && (P.dev & DEV_EXACT64)) { d.search = SearchKernel64::ORACLE; d.grid = (size_t)(B + 3) / 4; return; }
    if (dev_kernels && (P.dev & DEV_LITERAL) && !VALUE && P.N <= 40) { d.search = SearchKernel64::LITERAL; d.grid = (size_t)B; return; }
    const size_t total = (size_t)B * W;
    const bool o3 = dev_kernels && (P.dev & DEV_WAVES3) != 0;
    const size_t nslots = slots(A.n_cu, A.waves_per_simd, P.dev, dev_kernels);
    const size_t waves = grid(A.n_cu, A.waves_per_simd, false, P.dev, A.reserve_units, dev_kernels);
    const size_t g = total < waves ? total : waves;
    const bool pools = !o3 && search_pools(P, CAND, VALUE, packs_live_rows(P, B, A)) && (size_t)B >= 4 * nslots;
    d.order_stride = ((B + 7) / 8) * (pools ? 1 : W);
    if (!HI && search_is_static(P, B, A)) { d.search = SearchKernel64::CAPTURE_STATIC; d.grid = total; d.queues = 0; return; }
    d.queues = 8;
    int Pr_dev = P.dev;
    if (!VALUE && emits_in_pieces(P, A)) Pr_dev |= DEV_LAUNCH_CKPT;
    bool queues_built = false;
    if (CAND != CAND_TABLE) {
        if (packs_live_rows(P, B, A)) {
            queues_built = search_builds_queues(P, B, A) && !(P.dev & DEV_SEPARATE_QUEUES);
            d.rows_kernel = true; d.rows_with_queues = queues_built; d.rows_pool_arg = pools;
            if (queues_built) d.order = true;
            Pr_dev |= DEV_LAUNCH_LIVE_ROWS;
        }
    }
    if (!queues_built && search_builds_queues(P, B, A)) { d.build_queues_kernel = true; d.build_queues_rows = d.rows_kernel; d.order = true; }
    if (!HI && captures_trajectories(P, A)) { d.search = SearchKernel64::CAPTURE_QUEUES; d.grid = g; d.kernel_dev_bits = 0; return; }
    d.kernel_dev_bits = Pr_dev & ~P.dev;
    if (CAND == CAND_LATTICE && !VALUE && pools) {
        const size_t pwaves = grid(A.n_cu, A.waves_per_simd, true, P.dev, A.reserve_pool, dev_kernels);
        d.search = SearchKernel64::POOL; d.grid = (size_t)B < pwaves ? (size_t)B : pwaves;
        return;
    }
    d.grid = g;
    d.search = o3 ? SearchKernel64::UNITS_WAVES3 : SearchKernel64::UNITS;
}
// launch_emit<double> + launch_emit64
static void emit(const KP& P, const Args& A, bool dev_kernels, Did& d) {
    const bool HI = P.hi_order != 0;
    if (dev_kernels && (P.dev & DEV_EXACT64)) d.emit = EmitKernel64::ORACLE;
    else if (!HI && captures_trajectories(P, A)) d.emit = EmitKernel64::GATHER;
    else if (emits_in_pieces(P, A)) {
        d.emit = EmitKernel64::PIECES; d.S = seg_scenarios_per_block(P); d.lds = (size_t)d.S * (7 * (P.N + 1) + 4 * P.N) * 8;
    } else d.emit = EmitKernel64::ONE_PIECE;
}
static Did solve(const KP& P, int B, bool value, const Search64Env& env) {
    const Args A = carve(P, B, value, env);
    Did d{};
    // solve_impl: if (!exact64 && !counters_by_builder(kp, B, A)) hipMemsetAsync(work_counter)
    d.memset = !(P.dev & DEV_EXACT64) && !(search_is_static(P, B, A) || search_builds_queues(P, B, A));
    search(P, B, value, A, env.dev_kernels, d);
    emit(P, A, env.dev_kernels, d);
    return d;
}

}  // namespace parent

static void check_point(const KP& P, int B, bool value, const Search64Env& env) {
    g_P = P; g_B = B; g_value = value; g_env = env;
    ++n_points;
    const Search64Plan p = plan_search64(P, B, value, env);
    const parent::Did d = parent::solve(P, B, value, env);
    const parent::Args A = parent::carve(P, B, value, env);
    const int W = P.C / 64;
    const bool oracle = p.search_kernel == SearchKernel64::ORACLE, literal = p.search_kernel == SearchKernel64::LITERAL;
    const bool capture = p.search_kernel == SearchKernel64::CAPTURE_STATIC || p.search_kernel == SearchKernel64::CAPTURE_QUEUES;
    const bool pool = p.search_kernel == SearchKernel64::POOL;

    // every field against what the parent did
    CHECK(p.W == W && p.partials == W);                                    // solve_impl: W = value ? C / 64 : Wk, Wk = C / 64
    CHECK(p.reset_rec_count == (value && !(P.dev & DEV_EXACT64)));         // solve_impl: if (value) ... else if (!exact64) memset(rec_count)
    CHECK(p.ckpt_doubles == 0 && !p.reset_best_key);                       // the float plan's
    CHECK(p.search_kernel == d.search);
    CHECK(p.grid == d.grid && p.grid >= 1);
    CHECK(p.emit_kernel == d.emit);
    CHECK(p.seg_scenarios == d.S && p.seg_lds_bytes == d.lds);
    CHECK(p.live_rows == d.rows_kernel);
    CHECK(p.rows_build_queues == d.rows_with_queues);
    CHECK(p.separate_queue_builder == d.build_queues_kernel);
    CHECK(p.sorts_queues() == d.order);                                    // the search kernel's `order` argument is not null
    CHECK(p.launch_dev_bits == d.kernel_dev_bits);
    CHECK(!d.rows_kernel || d.rows_pool_arg == pool);                      // accel_rows_kernel's pool_units argument
    CHECK(!d.build_queues_kernel || d.build_queues_rows == p.live_rows);   // build_queues_kernel's row masks
    if (!oracle && !literal) {
        CHECK(p.queues == d.queues);
        CHECK(p.order_stride == d.order_stride);
    }
    CHECK(p.memset_counters == (literal ? false : d.memset));              // the one difference that is meant (see above)
    if (literal) CHECK(d.memset);
    // the workspace: never more than the parent carved, and exactly what the chosen kernels read
    CHECK((p.traj_doubles != 0) == capture);
    CHECK(p.traj_doubles == (capture ? (size_t)B * W * 9 * (P.N + 1) * 64 : 0) && (!capture || A.traj));
    // the checkpoint records: wherever the emit in pieces reads them -- and, measured, wherever the parent took them (without
    // them the arrays behind the partials lie elsewhere and the headline is 2 % slower), the developer kernels apart
    CHECK(p.ck_records == 0 || p.ck_records == (size_t)B * W);
    CHECK(p.emit_kernel != EmitKernel64::PIECES || p.ck_records != 0);
    CHECK((p.ck_records != 0) == (A.ck_records && !literal));
    CHECK(p.queue_order_words == (p.sorts_queues() ? (size_t)((B + 7) / 8) * 8 * W : 0) && (!p.queue_order_words || A.queue_order));
    // the order the builders write fits the words asked for: 8 queues of order_stride entries
    if (p.sorts_queues()) CHECK((size_t)8 * p.order_stride <= p.queue_order_words);

    // what held by convention
    CHECK((p.emit_kernel == EmitKernel64::GATHER) == capture);
    CHECK((p.emit_kernel == EmitKernel64::PIECES) == ((p.launch_dev_bits & DEV_LAUNCH_CKPT) != 0));
    CHECK((p.emit_kernel == EmitKernel64::ORACLE) == oracle);
    CHECK(((p.launch_dev_bits & DEV_LAUNCH_LIVE_ROWS) != 0) == p.live_rows);
    CHECK((p.launch_dev_bits & ~(DEV_LAUNCH_CKPT | DEV_LAUNCH_LIVE_ROWS)) == 0 && (p.launch_dev_bits & P.dev) == 0);
    if (!oracle && !literal) CHECK((p.queues == 0) == (p.search_kernel == SearchKernel64::CAPTURE_STATIC));
    CHECK(p.queues == 0 || p.queues == SEARCH64_QUEUES);
    const bool counters_used = p.queues != 0;                              // oracle, literal, static capture: none
    CHECK(p.memset_counters == (counters_used && !p.sorts_queues()));
    CHECK(!(p.rows_build_queues && p.separate_queue_builder) && (!p.rows_build_queues || p.live_rows));
    CHECK(!p.sorts_queues() || counters_used);
    if (pool) CHECK(P.cand_mode == CAND_LATTICE && !value && p.live_rows && !p.separate_queue_builder);
    if (capture) CHECK(!P.hi_order && P.n_rk4 == 4 && !p.live_rows);
    if (p.emit_kernel == EmitKernel64::PIECES) CHECK(!value && p.seg_scenarios >= 4 && p.seg_lds_bytes <= SEG_LDS_MAX);
    if (!env.dev_kernels) CHECK(!oracle && !literal && p.search_kernel != SearchKernel64::UNITS_WAVES3);

    // the grid: from search64_grid / search64_slots and from nowhere else
    if (counters_used) {
        const size_t items = pool ? (size_t)B : (size_t)B * W;
        const size_t waves = search64_grid(env.n_cu, env.waves_per_simd, pool ? Search64::POOL : Search64::UNITS, P.dev,
                                           pool ? env.reserve_pool : env.reserve_units, env.dev_kernels);
        CHECK(p.grid == (items < waves ? items : waves));
        CHECK(p.grid <= search64_slots(env.n_cu, env.waves_per_simd, P.dev, env.dev_kernels));
        if (pool) CHECK((size_t)B >= 4 * search64_slots(env.n_cu, env.waves_per_simd, P.dev, env.dev_kernels));
    } else if (p.search_kernel == SearchKernel64::CAPTURE_STATIC) {
        CHECK(p.grid == (size_t)B * W && p.grid <= (size_t)env.n_cu * 4);      // a wave per unit, one per SIMD at the most
    }
    // a refinement pass changes nothing the plan reads
    KP Q = P;
    Q.refine_it = 3;
    const Search64Plan q = plan_search64(Q, B, value, env);
    CHECK(q.search_kernel == p.search_kernel && q.emit_kernel == p.emit_kernel && q.grid == p.grid &&
          q.launch_dev_bits == p.launch_dev_bits && q.memset_counters == p.memset_counters && q.traj_doubles == p.traj_doubles &&
          q.ck_records == p.ck_records && q.queue_order_words == p.queue_order_words);
}

int main() {
    const int cands[] = {CAND_LATTICE, CAND_TABLE, CAND_RAMP_HOLD, CAND_TRACK};
    const int Bs[] = {1, 32, 256, 257, 1024, 1025, 4095, 4096, 6144, 6145, 65536}, Cs[] = {64, 256, 1024}, Ns[] = {4, 7, 8, 20, 40, 64};
    const int cus[] = {8, 256, 304};
    const int switches[] = {0, DEV_NO_SLICES, DEV_ALL_ROWS, DEV_NO_CAPTURE, DEV_KEEP_QUEUES, DEV_TRACE, DEV_NO_SEG_EMIT,
                            DEV_NO_QUEUE_ORDER, DEV_SEPARATE_QUEUES, DEV_WAVES3, DEV_NO_REFILL, DEV_NO_STEER_TABLE, DEV_WHOLE_COLUMNS,
                            DEV_NO_EARLY_EXIT, DEV_NO_RESERVE, DEV_EXACT64, DEV_LITERAL};
    struct Override { int traj_max, reserve_pool, reserve_units; };
    const Override overrides[] = {{-1, -1, -1}, {0, -1, -1}, {600, -1, -1}, {-1, 2, 3}};
    long kinds[7] = {0}, emits[4] = {0};
    for (int dev_kernels = 0; dev_kernels <= 1; ++dev_kernels)
    for (int dev : switches) {
        if (!dev_kernels && (dev & DEV_KERNEL_FLAGS)) continue;      // igt_create refuses them
        for (const Override& o : overrides)
        for (int n_cu : cus) for (int wps = 1; wps <= 2; ++wps) {
            Search64Env env{n_cu, wps, o.reserve_pool, o.reserve_units, o.traj_max, dev_kernels != 0};
            for (int cand : cands) for (int value = 0; value <= 1; ++value)
            for (int C : Cs) for (int N : Ns) for (int nrk = 2; nrk <= 4; nrk += 2) for (int hi = 0; hi <= 1; ++hi) {
                KP P{};
                P.cand_mode = cand; P.cost_mode = value; P.C = C; P.N = N; P.n_rk4 = nrk; P.hi_order = hi; P.dev = dev;
                P.G = C == 64 ? 8 : C == 256 ? 16 : 32;
                for (int B : Bs) {
                    check_point(P, B, value != 0, env);
                    const Search64Plan p = plan_search64(P, B, value != 0, env);
                    ++kinds[(int)p.search_kernel]; ++emits[(int)p.emit_kernel];
                }
            }
        }
    }
    // the sweep reaches every value of the two enums
    for (long k : kinds) if (k == 0) { std::fprintf(stderr, "a search kernel the sweep never selects\n"); return 1; }
    for (long k : emits) if (k == 0) { std::fprintf(stderr, "an emit kernel the sweep never selects\n"); return 1; }
    // the figures the write-up quotes: the headline (B = 4096, lattice, N = 20, C = 256, 256 compute units)
    {
        KP P{};
        P.cand_mode = CAND_LATTICE; P.C = 256; P.G = 16; P.N = 20; P.n_rk4 = 4;
        g_P = P; g_B = 4096; g_value = 0;
        const Search64Plan one = plan_search64(P, 4096, false, g_env = Search64Env{256, 2});
        CHECK(one.search_kernel == SearchKernel64::UNITS && one.grid == 2048 && one.emit_kernel == EmitKernel64::PIECES &&
              one.rows_build_queues && !one.memset_counters && one.seg_scenarios == 64);
        const Search64Plan four = plan_search64(P, 4096, false, g_env = Search64Env{256, 1});
        CHECK(four.search_kernel == SearchKernel64::POOL && four.grid == 992 && four.emit_kernel == EmitKernel64::ONE_PIECE &&
              four.order_stride == 512);
        const Search64Plan small = plan_search64(P, 32, false, g_env = Search64Env{256, 2});
        CHECK(small.search_kernel == SearchKernel64::CAPTURE_STATIC && small.grid == 128 && small.queues == 0 &&
              small.emit_kernel == EmitKernel64::GATHER && !small.memset_counters && small.queue_order_words == 0);
    }
    std::printf("search plan ok: %ld points\n", n_points);
    return 0;
}
