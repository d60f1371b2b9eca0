// Stand-alone check of the shape of the acceleration-row pass (csrc/igt_launch.h rows_scenarios_per_block / rows_groups and
// plan_search64's rows_threads; test_rows_shape_host.py builds the host side of it with the address / undefined-behaviour
// sanitizers and runs it).  For G in {4, 8, 16, 32, 64}, both workgroup sizes (one row per lane: no other mapping was kept)
// and every B from 1 to 9000:
//   * the launcher's group count covers B exactly: n_groups * per_block >= B > (n_groups - 1) * per_block, per_block being
//     what one workgroup of accel_rows_kernel indexes (waves * 64 lanes / lanes per scenario);
//   * rows_threads is 64 exactly where the row pass runs (live_rows) and solves overlap (waves_per_simd == 1), 256 everywhere
//     else, and never 64 without live_rows;
//   * DEV_WIDE_ROWS forces 256 and changes no other field of the plan.
#include "igt_launch.h"

#include <cstdio>
#include <cstdlib>

using namespace igt;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static bool same_but_rows_threads(const Search64Plan& a, const Search64Plan& b) {
    return a.W == b.W && a.search_kernel == b.search_kernel && a.grid == b.grid && a.queues == b.queues &&
           a.order_stride == b.order_stride && a.live_rows == b.live_rows && a.rows_build_queues == b.rows_build_queues &&
           a.separate_queue_builder == b.separate_queue_builder &&
           a.launch_dev_bits == b.launch_dev_bits && a.emit_kernel == b.emit_kernel && a.seg_scenarios == b.seg_scenarios &&
           a.seg_lds_bytes == b.seg_lds_bytes && a.traj_doubles == b.traj_doubles && a.ck_records == b.ck_records &&
           a.queue_order_words == b.queue_order_words && a.memset_counters == b.memset_counters;
}

int main() {
    const int Gs[] = {4, 8, 16, 32, 64}, threads[] = {ROWS_THREADS_WIDE, ROWS_THREADS_NARROW};
    CHECK(ROWS_THREADS_WIDE == 256 && ROWS_THREADS_NARROW == 64);
    long n_points = 0;
    // 1. the group count
    for (int G : Gs)
        for (int T : threads) {
            const int per_wave = 64 / G, per_block = (T / 64) * per_wave;      // one lane per (scenario, row)
            CHECK(per_wave >= 1 && per_wave * G == 64);                        // a scenario's lanes never straddle two waves
            CHECK(rows_scenarios_per_block(T, G) == per_block);
            for (int B = 1; B <= 9000; ++B) {
                const long n_groups = rows_groups(B, T, G);
                CHECK(n_groups >= 1 && n_groups * per_block >= B && B > (n_groups - 1) * per_block);
                ++n_points;
            }
        }
    // 2. the plan's rule, and the switch
    const int cands[] = {CAND_LATTICE, CAND_TABLE, CAND_RAMP_HOLD, CAND_TRACK}, Ns[] = {7, 8, 20}, cus[] = {8, 256};
    const int switches[] = {0, DEV_ALL_ROWS, DEV_NO_SLICES, DEV_NO_CAPTURE, DEV_SEPARATE_QUEUES, DEV_NO_REFILL, DEV_NO_RESERVE};
    long narrow = 0, narrow_pool = 0, narrow_units = 0;
    for (int G : Gs) for (int cand : cands) for (int N : Ns) for (int n_cu : cus) for (int wps = 0; wps <= 2; ++wps)
    for (int value = 0; value <= 1; ++value) for (int dev : switches) {
        KP P{};
        P.cand_mode = cand; P.cost_mode = value; P.G = cand == CAND_TABLE ? 1 : G; P.C = G * G; P.N = N; P.n_rk4 = 4; P.dev = dev;
        KP Q = P;
        Q.dev = dev | DEV_WIDE_ROWS;
        const Search64Env env{n_cu, wps};
        for (int B = 1; B <= 9000; ++B) {
            const Search64Plan p = plan_search64(P, B, value != 0, env), q = plan_search64(Q, B, value != 0, env);
            const bool rule = p.live_rows && env.waves_per_simd == 1;
            CHECK(p.rows_threads == (rule ? ROWS_THREADS_NARROW : ROWS_THREADS_WIDE));
            CHECK(p.live_rows || p.rows_threads == ROWS_THREADS_WIDE);
            CHECK(q.rows_threads == ROWS_THREADS_WIDE);
            CHECK(same_but_rows_threads(p, q));
            if (rule) { ++narrow; (p.search_kernel == SearchKernel64::POOL ? narrow_pool : narrow_units)++; }
            ++n_points;
        }
    }
    CHECK(narrow > 0 && narrow_pool > 0 && narrow_units > 0);      // the sweep reaches the one-wave shape under both searches
    CHECK((DEV_WIDE_ROWS & DEV_ENV_MASK) == DEV_WIDE_ROWS && DEV_WIDE_ROWS == 64);      // the environment may set it
    // the headline: B = 4096, lattice, 256 candidates, four solves in flight -> 1024 one-wave row workgroups and 8 builders
    {
        KP P{};
        P.cand_mode = CAND_LATTICE; P.C = 256; P.G = 16; P.N = 20; P.n_rk4 = 4;
        const Search64Plan four = plan_search64(P, 4096, false, Search64Env{256, 1}), one = plan_search64(P, 4096, false, Search64Env{256, 2});
        CHECK(four.rows_threads == ROWS_THREADS_NARROW && four.rows_build_queues && one.rows_threads == ROWS_THREADS_WIDE);
        CHECK(rows_groups(4096, one.rows_threads, P.G) == 256 && rows_groups(4096, four.rows_threads, P.G) == 1024);
    }
    std::printf("rows shape ok: %ld points\n", n_points);
    return 0;
}
