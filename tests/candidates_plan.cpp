// Stand-alone check of the plan of a solve on per-scenario candidate sets (csrc/igt_launch.h plan_candidates64;
// test_candidates_host.py builds the host side of it with the address / undefined-behaviour sanitizers and runs it): over
// batch sizes, candidate counts, horizons and both costs -- one wave per unit on a plain grid, no queues, prelude, launch-time
// bits, trajectories, records, queue order or counter memset; the one-piece emit at priority 0 at every batch size; the staged
// kernel exactly for the progress cost with a slab of at most an eighth of a compute unit's LDS (N <= 20), the direct one
// otherwise; and plan_search64 never names either kernel.
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

int main() {
    const int Bs[] = {1, 6, 8, 255, 256, 257, 1024, 4096, 8192, 65536}, Cs[] = {64, 128, 256, 1024};
    const int Ns[] = {1, 8, 13, 19, 20, 21, 40, 64, 100};
    long n = 0;
    for (int B : Bs)
        for (int C : Cs)
            for (int N : Ns)
                for (int value = 0; value < 2; ++value) {
                    KP P{};
                    P.C = C; P.N = N; P.G = 16; P.cand_mode = CAND_TABLE; P.n_rk4 = 4;
                    const Search64Plan p = plan_candidates64(P, B, value != 0);
                    CHECK(p.W == C / 64 && p.grid == (size_t)B * (size_t)(C / 64));
                    CHECK(p.queues == 0 && !p.live_rows && !p.rows_build_queues && !p.separate_queue_builder && !p.sorts_queues());
                    CHECK(p.launch_dev_bits == 0 && !p.memset_counters && p.emit_priority == 0);
                    CHECK(p.emit_kernel == EmitKernel64::ONE_PIECE && p.seg_scenarios == 0 && p.seg_lds_bytes == 0);
                    CHECK(p.traj_doubles == 0 && p.ck_records == 0 && p.queue_order_words == 0);
                    const bool fits = (size_t)2 * N * 64 * 8 <= (size_t)20 * 1024;
                    CHECK(fits == (N <= 20));
                    CHECK(p.search_kernel == (!value && fits ? SearchKernel64::CANDIDATES_STAGED : SearchKernel64::CANDIDATES_DIRECT));
                    // the table family's own plan keeps to the kernels it had, on every chip and concurrency
                    for (int n_cu : {8, 256})
                        for (int w : {1, 2}) {
                            const Search64Plan q = plan_search64(P, B, value != 0, Search64Env{n_cu, w});
                            CHECK(q.search_kernel != SearchKernel64::CANDIDATES_STAGED && q.search_kernel != SearchKernel64::CANDIDATES_DIRECT);
                        }
                    ++n;
                }
    // the figures the write-up quotes
    CHECK(cand_slab_doubles(20) * 8 == 20480 && CAND_SLAB_MAX_BYTES == 20480 && 8 * CAND_SLAB_MAX_BYTES == CAND_LDS_BUDGET);
    CHECK(cand_table_doubles(256, 20) * 8 == 81920 && (size_t)4096 * cand_table_doubles(256, 20) * 8 == 335544320);
    std::printf("candidates plan ok: %ld points\n", n);
    return 0;
}
