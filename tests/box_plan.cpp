// Stand-alone check of the plan of a solve under the rectangle (OBCA) collision model (csrc/igt_launch.h plan_box64, box_model;
// test_box_host.py builds the host side of it with the address / undefined-behaviour sanitizers and runs it): over batch sizes,
// candidate counts, horizons, families and both costs -- search_box_f64_kernel with one wave per unit on a plain grid, no
// queues, prelude, launch-time bits, trajectories, records, queue order or counter memset; the one-piece emit at priority 0 at
// every batch size; plan_search64 and plan_candidates64 never ask for the kernel; the model's figures and what it refuses; the
// LDS table holds every (obstacle, node) the header allows.
#include "igt_launch.h"
#include "igt_roll_options.h"
#include "igtmpc.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace igt;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// the option is a bit of its own, search and rollout-all derive what they derived, and the pool's table is refused with it
static_assert(ROLL_BOX == 1u << 10 && (ROLL_BOX & (ROLL_POOL | ROLL_ALL | ROLL_LEAVE_CKPT | ROLL_RESUME | ROLL_NO_XY | ROLL_STEP_TABLE)) == 0, "a bit of its own");
static_assert(roll_lean(ROLL_SEARCH | ROLL_BOX) && !roll_lean(ROLL_ALL | ROLL_BOX), "lean in the search, verdict bits in rollout-all");
static_assert(roll_supported(ROLL_SEARCH | ROLL_BOX | ROLL_STEER_TABLE | ROLL_NO_XY) && roll_supported(ROLL_ALL | ROLL_BOX), "the builds");
static_assert(!roll_supported(ROLL_POOL | ROLL_STEP_TABLE | ROLL_BOX), "no pooled box search");

int main() {
    const int Bs[] = {0, 1, 6, 8, 255, 256, 257, 1024, 4096, 8192, 65536}, Cs[] = {64, 128, 256, 1024};
    const int Ns[] = {1, 8, 13, 20, 40, 64}, cands[] = {CAND_LATTICE, CAND_TABLE, CAND_RAMP_HOLD, CAND_TRACK};
    long n = 0;
    for (int B : Bs)
        for (int C : Cs)
            for (int N : Ns)
                for (int cand : cands)
                    for (int value = 0; value < 2; ++value) {
                        KP P{};
                        P.C = C; P.N = N; P.G = C == 64 ? 8 : C == 256 ? 16 : C == 1024 ? 32 : 0; P.cand_mode = cand; P.n_rk4 = 4; P.n_obs = 4;
                        const Search64Plan p = plan_box64(P, B, value != 0);
                        CHECK(p.box && p.search_kernel == SearchKernel64::UNITS && p.emit_kernel == EmitKernel64::ONE_PIECE);
                        CHECK(p.W == C / 64 && p.partials == p.W && p.grid == (size_t)B * (size_t)(C / 64));
                        CHECK(p.queues == 0 && !p.live_rows && !p.rows_build_queues && !p.separate_queue_builder && !p.sorts_queues());
                        CHECK(p.launch_dev_bits == 0 && !p.memset_counters && p.emit_priority == 0);
                        CHECK(p.seg_scenarios == 0 && p.seg_lds_bytes == 0);
                        CHECK(p.traj_doubles == 0 && p.ck_records == 0 && p.queue_order_words == 0);
                        CHECK(p.reset_rec_count == (value != 0));
                        if (B > 0 && P.G > 0)
                            for (int n_cu : {8, 256})
                                for (int w : {1, 2})
                                    CHECK(!plan_search64(P, B, value != 0, Search64Env{n_cu, w}).box);
                        CHECK(!plan_candidates64(P, B, value != 0).box);
                        ++n;
                    }
    // the model: the reference's vehicle, d_min = 0
    BoxModel m{};
    CHECK(!box_model(4.47, 2.0, 0.0, &m));                // nullptr: nothing to refuse
    CHECK(m.h0 == 2.235 && m.h1 == 1.0 && m.dsafe == 1e-6);
    const double gate = 1e-6 + 2.0 * std::sqrt(2.235 * 2.235 + 1.0);
    CHECK(std::fabs(m.gate2 - gate * gate) < 1e-12 && gate > 4.89 && gate < 4.90);
    CHECK(!box_model(4.47, 2.0, 1.5, &m) && m.dsafe == 1.5 + 1e-6);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    BoxModel keep = m;
    for (double bad : {0.0, -1.0, inf, -inf, nan}) {
        const char *l = box_model(bad, 2.0, 0.0, &m), *w = box_model(4.47, bad, 0.0, &m);
        CHECK(l && std::strstr(l, "length") && w && std::strstr(w, "width"));      // the refusal names the cause
        if (bad != 0.0) {
            const char* d = box_model(4.47, 2.0, bad, &m);
            CHECK(d && std::strstr(d, "d_box"));
        }
    }
    CHECK(m.h0 == keep.h0 && m.gate2 == keep.gate2);      // a refused model writes nothing
    // the unit's LDS table: every (obstacle, node) of the largest problem, 8 KB and a header
    CHECK(BOX_TAB_MAX_ENTRIES == IGT_MAX_OBS * IGT_MAX_N && BOX_TAB_FIELDS == 4);
    CHECK(BOX_TAB_DOUBLES * sizeof(double) == 8192 + BOX_TAB_HEADER * sizeof(double));
    std::printf("box plan ok: %ld points\n", n);
    return 0;
}
