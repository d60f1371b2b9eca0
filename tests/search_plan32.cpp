// Stand-alone check of the plan of a float solve (csrc/igt_launch.h plan_search32; test_search_plan_host.py builds the host
// side of it with the address / undefined-behaviour sanitizers and runs it).
//
// Before the plan, one question was answered in three places: solve_impl<float> decided the units, the partials, the pieces of
// the emit and the workspace behind `sizeof(T) == 4` tests, launch_search_fast re-derived the queue builder, the kernel build, the
// grid and the incumbents from pointers and SolveArgs fields, launch_emit_fast chose its kernel by a pointer.  This program
// restates those three places as they were written -- pointers as booleans, the returns in their order -- and compares every
// field of the plan, and every size solve_impl carves from it, with what they did, over
//   the four families x both costs x B in {1, 32, 2048, 2049, 2304, 6144, 6145, 9000, 65536} x C in {64, 192, 256, 1024, 65536}
//   x N in {3, 4, 6, 7, 8, 10, 20, 33, 40} x hi_order x n_cu in {8, 256, 304} x waves_per_simd in {1, 2}
//   x {no switch, DEV_NO_SLICES, DEV_STEER_SLICES, DEV_NO_BOUND, DEV_NO_QUEUE_ORDER, DEV_TRACE, DEV_WAVES3 alone}
//   x IGT_DEV_CKPT in {unset, 0, 1, 2, 3, 4, 5, 8}
// and both kinds of library; DEV_WAVES3 only with the library that carries its kernels: igt_create refuses it otherwise.
// One difference is meant.  With DEV_WAVES3 the search launcher took the 3-waves-per-SIMD build first -- it leaves no
// checkpoints -- while solve_impl had carved them and launch_emit_fast, seeing the pointer, rolled the winner's pieces from
// checkpoints nobody had written (B <= 2048 or an IGT_DEV_CKPT override; no test ran such a solve).  The plan gives that build
// one piece and no checkpoints; both sides are asserted at those points.
// Then what held by convention only: emit in pieces <=> the search left checkpoints <=> checkpoints were carved <=> more than one
// piece; the pieces divide the horizon; the host zeroes the counters exactly where no builder does; the builder runs only within
// its capacity and on order words that were taken and hold its 8 queues; incumbents only where the device's accel_units holds;
// the grid is min(units, slots).
#include "igt_launch.h"

#include <cstdio>
#include <cstdlib>

using namespace igt;

static long n_points = 0;
static KP g_P;
static int g_B, g_value;
static Search32Env g_env;

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::fprintf(stderr, "%s:%d: %s\n  cand %d value %d B %d C %d G %d N %d hi %d dev %d n_cu %d wps %d dev_ckpt %d "     \
                         "dev_kernels %d\n", __FILE__, __LINE__, #cond, g_P.cand_mode, g_value, g_B, g_P.C, g_P.G, g_P.N,          \
                         g_P.hi_order, g_P.dev, g_env.n_cu, g_env.waves_per_simd, g_env.dev_ckpt, (int)g_env.dev_kernels);       \
            std::exit(1);                                                                                                        \
        }                                                                                                                        \
    } while (0)

// ---- the parent's three places, restated ----
namespace parent {

struct Args {      // SolveArgs<float>: the pointers the launchers tested, as "not null"; the numbers they read; the sizes carved
    bool ckpt, queue_order;
    int ck_parts, n_cu, waves_per_simd;
    size_t Wk, W;                                           // units and partials per scenario
    size_t part_J_doubles, part_c_words, counter_words;     // take<double>, take<int32_t>, take<unsigned>
    size_t ckpt_doubles, queue_order_words, unit_seg;
    bool memset_rec_count, memset_best_key;                 // solve_impl's pass loop
};
// solve_impl<float>: what it decided and carved
static Args carve(const KP& P, int B, bool value, const Search32Env& env) {
    Args A{};
    const bool compact = value;                             // value && sizeof(T) == 4
    const size_t Wk = ((size_t)P.C + 127) / 128;
    const size_t W = compact ? 1 : Wk;                      // (value ? C / 64 : Wk) is the double path's
    int ck_parts = 1;
    if (B <= 2048 && P.N % 4 == 0 && P.N >= 8) ck_parts = 4;
    else if (B <= 2048 && P.N % 2 == 0 && P.N >= 4) ck_parts = 2;
    if (env.dev_ckpt >= 0) {
        const int v = env.dev_ckpt;
        if (v >= 1 && v <= 4 && P.N % v == 0 && P.N >= 2 * v) ck_parts = v;
    }
    const bool use_ckpt = ck_parts > 1;
    const size_t queue_order_words = B <= 6144 ? (size_t)((B + 7) / 8) * 8 * Wk : 0;
    const bool trace = (P.dev & DEV_TRACE) != 0;
    A.Wk = Wk; A.W = W;
    A.part_J_doubles = (size_t)B * W + (size_t)B;           // PartJTail<float>::doubles
    A.part_c_words = (size_t)B * W;
    A.counter_words = 1024 + (trace ? (size_t)((B + 7) / 8) * 8 * Wk * 8 : 0);
    A.ckpt = use_ckpt;
    A.ckpt_doubles = use_ckpt ? (size_t)(ck_parts - 1) * B * Wk * (12 * 128) : 0;
    A.queue_order = queue_order_words != 0;
    A.queue_order_words = queue_order_words;
    A.unit_seg = value ? (size_t)B * Wk : 0;
    A.ck_parts = ck_parts;
    A.n_cu = env.n_cu; A.waves_per_simd = env.waves_per_simd;
    A.memset_rec_count = A.memset_best_key = compact;
    return A;
}
static bool search_builds_queues(const KP& P, int B, const Args& A) {
    const int W = (P.C + 127) / 128;
    return A.queue_order && W <= 256 && ((B + 7) / 8) * W <= 1024 * 2 && !(P.dev & DEV_NO_QUEUE_ORDER);
}

struct Did {      // what the launchers enqueued
    SearchKernel32 search; size_t grid; int queues; bool order; int order_stride; int kernel_dev_bits;
    bool memset_incumbents, build_queues_kernel; int builder_dev_bits; int kernel_ck_parts;
    EmitKernel32 emit; size_t emit_grid; int emit_parts;
    bool memset_counters;
};
// launch_search_fast<CAND, HI, VALUE>, return by return
static void search(const KP& P, int B, bool VALUE, const Args& A, bool dev_kernels, Did& d) {
    const int CAND = P.cand_mode;
    const int W = (P.C + 127) / 128;
    const size_t total = (size_t)B * W;
    const bool o3 = dev_kernels && (P.dev & DEV_WAVES3) != 0;
    const size_t slots = (size_t)A.n_cu * 4 * (o3 ? 3 : (A.waves_per_simd == 1 ? 1 : 2));
    d.grid = total < slots ? total : slots;
    d.order = false;
    d.order_stride = ((B + 7) / 8) * W;
    d.queues = 8;
    d.kernel_ck_parts = A.ck_parts;
    int Pr_dev = P.dev;
    if (CAND == CAND_TRACK && !VALUE) {
        if (P.G * P.G == P.C && W * 128 == P.C && P.G >= 16 && P.G <= 64 &&
            !(P.dev & (DEV_NO_SLICES | DEV_STEER_SLICES | DEV_NO_BOUND)) && W > 1) {
            d.memset_incumbents = true;
            Pr_dev |= DEV_LAUNCH_INCUMBENTS;
        }
    }
    if (search_builds_queues(P, B, A)) { d.build_queues_kernel = true; d.builder_dev_bits = Pr_dev & ~P.dev; d.order = true; }
    d.kernel_dev_bits = Pr_dev & ~P.dev;
    if (o3) { d.search = SearchKernel32::WAVES3; return; }
    if (A.ckpt && A.ck_parts > 1) { d.search = SearchKernel32::CHECKPOINTS; return; }
    if (CAND == CAND_TRACK) { d.search = SearchKernel32::TRACK; return; }
    d.search = SearchKernel32::UNITS;
}
// launch_emit_fast<CAND, HI>
static void emit(int B, const Args& A, Did& d) {
    if (A.ckpt) { d.emit = EmitKernel32::PIECES; d.emit_grid = ((size_t)B * A.ck_parts + 63) / 64; d.emit_parts = A.ck_parts; return; }
    d.emit = EmitKernel32::ONE_PIECE; d.emit_grid = (size_t)(B + 63) / 64; d.emit_parts = 1;
}
static Did solve(const KP& P, int B, bool value, const Search32Env& env) {
    const Args A = carve(P, B, value, env);
    Did d{};
    d.memset_counters = !search_builds_queues(P, B, A);      // host_zeroes_counters, on both branches of the pass loop
    search(P, B, value, A, env.dev_kernels, d);
    emit(B, A, d);
    return d;
}

}  // namespace parent

// igt_kernels.hip accel_units<CAND>(P, W), restated: where the tracking family's units are acceleration rows
static bool accel_units(const KP& P, int W) {
    return P.cand_mode == CAND_TRACK && P.G * P.G == P.C && W * 128 == P.C && P.G >= 16 && P.G <= 64 &&
           !(P.dev & (DEV_NO_SLICES | DEV_STEER_SLICES));
}

static long n_meant = 0;

static void check_point(const KP& P, int B, bool value, const Search32Env& env) {
    g_P = P; g_B = B; g_value = value; g_env = env;
    ++n_points;
    const Search32Plan p = plan_search32(P, B, value, env);
    const parent::Did d = parent::solve(P, B, value, env);
    const parent::Args A = parent::carve(P, B, value, env);
    const int W = (P.C + 127) / 128;
    const size_t total = (size_t)B * W;
    const bool o3 = p.search_kernel == SearchKernel32::WAVES3;
    // the one difference that is meant (see above): the parent's _o3 search beside checkpoints it never wrote
    const bool meant = o3 && A.ckpt;

    // every field against what the parent did
    CHECK(p.W == W && (size_t)p.W == A.Wk && (size_t)p.partials == A.W);
    CHECK(p.search_kernel == d.search);
    CHECK(p.grid == d.grid && p.grid >= 1);
    CHECK(p.queues == d.queues && p.order_stride == d.order_stride);
    CHECK(p.builds_queues == d.build_queues_kernel && p.builds_queues == d.order);      // the kernel's `order` argument is not null
    CHECK(p.launch_dev_bits == d.kernel_dev_bits && (!d.build_queues_kernel || d.builder_dev_bits == p.launch_dev_bits));
    CHECK(p.incumbents() == d.memset_incumbents);
    CHECK(p.memset_counters == d.memset_counters);
    CHECK(p.reset_rec_count == A.memset_rec_count && p.reset_best_key == A.memset_best_key);
    CHECK(p.queue_order_words == A.queue_order_words);
    if (!meant) {
        CHECK(p.ck_parts == A.ck_parts && p.ck_parts == d.kernel_ck_parts && p.ck_parts == d.emit_parts);
        CHECK(p.ckpt_doubles == A.ckpt_doubles && (p.ckpt_doubles != 0) == A.ckpt);
        CHECK(p.emit_kernel == d.emit && p.emit_grid == d.emit_grid);
    } else {
        ++n_meant;
        CHECK(env.dev_kernels && (P.dev & DEV_WAVES3));
        CHECK(d.search == SearchKernel32::WAVES3 && d.emit == EmitKernel32::PIECES && A.ck_parts > 1 && A.ckpt_doubles != 0);
        CHECK(p.ck_parts == 1 && p.ckpt_doubles == 0 && p.emit_kernel == EmitKernel32::ONE_PIECE && p.emit_grid == (size_t)(B + 63) / 64);
    }
    // the sizes solve_impl carves from the plan, in the parent's order: partials and incumbents, part_c, (cpar: [B, 4]), the
    // counters and the trace, checkpoints, queue order, (the value path's records: [B, C] each), unit_seg
    CHECK(PartJTail<float>(nullptr, B, p.partials, P.G).doubles(p.ck_records != 0) == A.part_J_doubles);
    CHECK((size_t)B * p.partials == A.part_c_words);
    CHECK(WORK_COUNTER_WORDS + ((P.dev & DEV_TRACE) ? (size_t)((B + 7) / 8) * 8 * p.W * 8 : 0) == A.counter_words);
    CHECK((value ? (size_t)B * p.W : 0) == A.unit_seg);
    CHECK(p.ck_records == 0 && p.traj_doubles == 0);
    // the order words are taken for every B <= 6144, also where no builder runs
    CHECK((p.queue_order_words != 0) == (B <= 6144) && (!p.queue_order_words || p.queue_order_words == (size_t)((B + 7) / 8) * 8 * W));

    // what held by convention
    const bool pieces = p.emit_kernel == EmitKernel32::PIECES;
    CHECK(pieces == (p.search_kernel == SearchKernel32::CHECKPOINTS));
    CHECK(pieces == (p.ckpt_doubles != 0) && pieces == (p.ck_parts > 1));
    CHECK(p.ckpt_doubles == (pieces ? (size_t)(p.ck_parts - 1) * total * SEG_UNIT_DOUBLES : 0));
    CHECK(p.ck_parts >= 1 && p.ck_parts <= SEG_MAX_PARTS && P.N % p.ck_parts == 0 && P.N >= 2 * p.ck_parts);
    CHECK(p.emit_grid == ((size_t)B * p.ck_parts + 63) / 64);
    CHECK(p.memset_counters == !p.builds_queues);
    if (p.builds_queues) {
        CHECK(p.queue_order_words != 0 && p.W <= 256 && (size_t)p.order_stride <= (size_t)QB_THREADS * QB_TRIPS);
        CHECK((size_t)8 * p.order_stride <= p.queue_order_words);
        CHECK(!(P.dev & DEV_NO_QUEUE_ORDER));
    }
    if (p.incumbents()) CHECK(P.cand_mode == CAND_TRACK && !value && accel_units(P, W) && W > 1 && !(P.dev & DEV_NO_BOUND));
    CHECK((p.launch_dev_bits & ~DEV_LAUNCH_INCUMBENTS) == 0 && (p.launch_dev_bits & P.dev) == 0);
    const size_t slots = (size_t)env.n_cu * 4 * (o3 ? 3 : env.waves_per_simd == 1 ? 1 : 2);
    CHECK(p.grid <= slots && p.grid == (total < slots ? total : slots));
    CHECK(p.queues == SEARCH32_QUEUES);
    CHECK(o3 == (env.dev_kernels && (P.dev & DEV_WAVES3) != 0));
    CHECK((p.search_kernel == SearchKernel32::TRACK) == (!o3 && !pieces && P.cand_mode == CAND_TRACK));
    CHECK(p.partials == (value ? 1 : W) && p.reset_rec_count == value && p.reset_best_key == value);
    // a refinement pass changes nothing the plan reads
    KP Q = P;
    Q.refine_it = 3;
    const Search32Plan q = plan_search32(Q, B, value, env);
    CHECK(q.search_kernel == p.search_kernel && q.emit_kernel == p.emit_kernel && q.grid == p.grid && q.emit_grid == p.emit_grid &&
          q.launch_dev_bits == p.launch_dev_bits && q.memset_counters == p.memset_counters && q.ck_parts == p.ck_parts &&
          q.ckpt_doubles == p.ckpt_doubles && q.queue_order_words == p.queue_order_words && q.builds_queues == p.builds_queues);
}

int main() {
    const int cands[] = {CAND_LATTICE, CAND_TABLE, CAND_RAMP_HOLD, CAND_TRACK};
    const int Bs[] = {1, 32, 2048, 2049, 2304, 6144, 6145, 9000, 65536}, Cs[] = {64, 192, 256, 1024, 65536};
    const int Ns[] = {3, 4, 6, 7, 8, 10, 20, 33, 40};
    const int cus[] = {8, 256, 304};
    const int switches[] = {0, DEV_NO_SLICES, DEV_STEER_SLICES, DEV_NO_BOUND, DEV_NO_QUEUE_ORDER, DEV_TRACE, DEV_WAVES3};
    const int ckpts[] = {-1, 0, 1, 2, 3, 4, 5, 8};
    long kinds[4] = {0}, emits[2] = {0}, incumbents = 0, no_builder_small = 0;
    for (int dev_kernels = 0; dev_kernels <= 1; ++dev_kernels)
    for (int dev : switches) {
        if (!dev_kernels && (dev & DEV_KERNEL_FLAGS)) continue;      // igt_create refuses them
        for (int ck : ckpts) for (int n_cu : cus) for (int wps = 1; wps <= 2; ++wps) {
            Search32Env env{n_cu, wps, ck, dev_kernels != 0};
            for (int cand : cands) for (int value = 0; value <= 1; ++value)
            for (int C : Cs) for (int N : Ns) for (int hi = 0; hi <= 1; ++hi) {
                KP P{};
                P.cand_mode = cand; P.cost_mode = value; P.C = C; P.N = N; P.n_rk4 = 4; P.hi_order = hi; P.dev = dev;
                P.G = C == 64 ? 8 : C == 192 ? 14 : C == 256 ? 16 : C == 1024 ? 32 : 256;      // 192: no square, the odd chunk count
                for (int B : Bs) {
                    check_point(P, B, value != 0, env);
                    const Search32Plan p = plan_search32(P, B, value != 0, env);
                    ++kinds[(int)p.search_kernel]; ++emits[(int)p.emit_kernel];
                    incumbents += p.incumbents();
                    no_builder_small += p.queue_order_words != 0 && !p.builds_queues;
                }
            }
        }
    }
    // the sweep reaches every value of the two enums, the incumbents, the order words without a builder and the meant difference
    for (long k : kinds) if (k == 0) { std::fprintf(stderr, "a search kernel the sweep never selects\n"); return 1; }
    for (long k : emits) if (k == 0) { std::fprintf(stderr, "an emit kernel the sweep never selects\n"); return 1; }
    if (!incumbents || !no_builder_small || !n_meant) { std::fprintf(stderr, "a case the sweep never reaches\n"); return 1; }
    // the figures the write-up quotes: lattice, N = 20, C = 256, 256 compute units
    {
        KP P{};
        P.cand_mode = CAND_LATTICE; P.C = 256; P.G = 16; P.N = 20; P.n_rk4 = 4;
        g_P = P; g_B = 4096; g_value = 0;
        const Search32Plan big = plan_search32(P, 4096, false, g_env = Search32Env{256, 2});
        CHECK(big.W == 2 && big.search_kernel == SearchKernel32::UNITS && big.grid == 2048 && big.emit_kernel == EmitKernel32::ONE_PIECE &&
              big.emit_grid == 64 && big.builds_queues && !big.memset_counters && big.ck_parts == 1 && big.order_stride == 1024);
        g_B = 1024;
        const Search32Plan small = plan_search32(P, 1024, false, g_env = Search32Env{256, 2});
        CHECK(small.search_kernel == SearchKernel32::CHECKPOINTS && small.grid == 2048 && small.emit_kernel == EmitKernel32::PIECES &&
              small.ck_parts == 4 && small.emit_grid == 64 && small.ckpt_doubles == (size_t)3 * 2048 * 1536 && small.builds_queues);
        g_B = 9000;
        const Search32Plan huge = plan_search32(P, 9000, false, g_env = Search32Env{256, 1});
        CHECK(huge.grid == 1024 && !huge.builds_queues && huge.memset_counters && huge.queue_order_words == 0);
    }
    std::printf("search plan32 ok: %ld points\n", n_points);
    return 0;
}
