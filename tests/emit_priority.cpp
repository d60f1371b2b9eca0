// Stand-alone check of plan_search64's emit_priority (csrc/igt_launch.h): the wave priority the one-piece float64 emit raises
// itself to when solves overlap.  test_emit_priority_host.py builds the host side of it with the address / undefined-behaviour
// sanitizers and runs it.  Over the grid of rows_shape.cpp -- G in {4, 8, 16, 32, 64}, the four families, N in {7, 8, 20}, 8 and
// 256 compute units, zero to two waves per SIMD, both costs, the switches that move the plan -- and batch sizes around every bound
// the plan has (256, 1024, 4096, 6144, 8192):
//   * emit_priority is EMIT_PRIORITY_OVERLAP exactly where the search kernel is POOL, the emit kernel ONE_PIECE, solves overlap
//     (waves_per_simd == 1) and DEV_EMIT_PRIO0 is off, else 0 -- so never for a family other than the lattice, whose emit kernel
//     alone has the raised build (launch_emit64);
//   * DEV_EMIT_PRIO0 changes no other field of the plan.
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

static bool same_but_emit_priority(const Search64Plan& a, const Search64Plan& b) {
    return a.W == b.W && a.search_kernel == b.search_kernel && a.grid == b.grid && a.queues == b.queues &&
           a.order_stride == b.order_stride && a.live_rows == b.live_rows && a.rows_build_queues == b.rows_build_queues &&
           a.rows_threads == b.rows_threads && a.separate_queue_builder == b.separate_queue_builder &&
           a.launch_dev_bits == b.launch_dev_bits && a.emit_kernel == b.emit_kernel && a.seg_scenarios == b.seg_scenarios &&
           a.seg_lds_bytes == b.seg_lds_bytes && a.traj_doubles == b.traj_doubles && a.ck_records == b.ck_records &&
           a.queue_order_words == b.queue_order_words && a.memset_counters == b.memset_counters;
}

int main() {
    const int Gs[] = {4, 8, 16, 32, 64};
    const int cands[] = {CAND_LATTICE, CAND_TABLE, CAND_RAMP_HOLD, CAND_TRACK}, Ns[] = {7, 8, 20}, cus[] = {8, 256};
    const int switches[] = {0, DEV_ALL_ROWS, DEV_NO_SLICES, DEV_NO_CAPTURE, DEV_SEPARATE_QUEUES, DEV_NO_REFILL, DEV_NO_RESERVE,
                            DEV_WIDE_ROWS, DEV_NO_QUEUE_ORDER};
    const int around[] = {1, 256, 1024, 4096, 6144, 8192};
    CHECK(EMIT_PRIORITY_OVERLAP >= 1 && EMIT_PRIORITY_OVERLAP <= 3);      // what s_setprio takes
    long n_points = 0, raised = 0, one_piece_not_raised = 0;
    for (int G : Gs) for (int cand : cands) for (int N : Ns) for (int n_cu : cus) for (int wps = 0; wps <= 2; ++wps)
    for (int value = 0; value <= 1; ++value) for (int dev : switches) {
        KP P{};
        P.cand_mode = cand; P.cost_mode = value; P.G = cand == CAND_TABLE ? 1 : G; P.C = G * G; P.N = N; P.n_rk4 = 4; P.dev = dev;
        KP Q = P;
        Q.dev = dev | DEV_EMIT_PRIO0;
        const Search64Env env{n_cu, wps};
        for (int centre : around) for (int B = centre > 40 ? centre - 40 : 1; B <= centre + 40; ++B) {
            const Search64Plan p = plan_search64(P, B, value != 0, env), q = plan_search64(Q, B, value != 0, env);
            const bool rule = p.search_kernel == SearchKernel64::POOL && p.emit_kernel == EmitKernel64::ONE_PIECE && env.waves_per_simd == 1;
            CHECK(p.emit_priority == (rule ? EMIT_PRIORITY_OVERLAP : 0));
            CHECK(p.emit_priority == 0 || (cand == CAND_LATTICE && !value));      // the build launch_emit64 has
            CHECK(q.emit_priority == 0);
            CHECK(same_but_emit_priority(p, q));
            if (rule) ++raised;
            else if (p.emit_kernel == EmitKernel64::ONE_PIECE && env.waves_per_simd == 1) ++one_piece_not_raised;
            ++n_points;
        }
    }
    CHECK(raised > 0 && one_piece_not_raised > 0);      // the sweep reaches both sides of the rule under overlap
    CHECK((DEV_EMIT_PRIO0 & DEV_ENV_MASK) == DEV_EMIT_PRIO0 && DEV_EMIT_PRIO0 == 128);      // the environment may set it
    // the headline: B = 4096, lattice, 256 candidates -- raised with four and three solves in flight, not alone; the tracking family not
    {
        KP P{};
        P.cand_mode = CAND_LATTICE; P.C = 256; P.G = 16; P.N = 20; P.n_rk4 = 4;
        CHECK(plan_search64(P, 4096, false, Search64Env{256, 1}).emit_priority == EMIT_PRIORITY_OVERLAP);
        CHECK(plan_search64(P, 4096, false, Search64Env{256, 2}).emit_priority == 0);
        CHECK(plan_search64(P, 65536, false, Search64Env{256, 2}).emit_priority == 0);
        P.cand_mode = CAND_TRACK;
        const Search64Plan track = plan_search64(P, 4096, false, Search64Env{256, 1});
        CHECK(track.emit_kernel == EmitKernel64::ONE_PIECE && track.emit_priority == 0);
    }
    std::printf("emit priority ok: %ld points\n", n_points);
    return 0;
}
