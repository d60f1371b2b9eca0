// Prints the plan the library would choose for each station of the handle walks (tests/handle_walk_cases.py): a host-only
// program over csrc/igt_launch.h, built with the address / undefined-behaviour sanitizers and run by test_handle_walk_host.py
// (256 compute units) and by test_gpu_handle_walk.py (the device's own count).
//
//   handle_walk_plan <n_cu> <item> ...      item = dtype,family,cost,N,C,B,concurrency,dev,own
//     dtype f64 | f32; family lattice | table | ramp_hold | track; cost progress | value_net; dev: IGT_DEV_FLAGS of the handle;
//     own 1: the call brings per-scenario candidates U[B,C,2,N] (solve_candidates)
//
// One line per item: the item, then every field of Search64Plan / Search32Plan as name=value.  The plan comes from the header's
// plan_search64, plan_candidates64 and plan_search32, called the way solve_impl (csrc/igt_api.hip) calls them: KP::G as make_kp
// sets it, waves_per_simd = 1 from three solves in flight, the shipped library (no developer kernels), no developer sweeps.
// The plans themselves are not restated.  What this program does restate, because it lives in csrc/igt_api.hip behind the
// handle and not in the header, is how solve_impl and make_kp fill the plans' inputs -- three lines, marked below; if one of them
// changes there, it has to change here:
//   * waves_per_simd = 1 from three solves in flight, else 2 (solve_impl);
//   * KP::G = 1 for the table family, else sqrt(C) (make_kp);
//   * KP::hi_order = 0: the stations keep the default limits and n_rk4 = 4, for which make_kp's rule gives
//     h v (0.7 / l_r + 0.25) = 0.099 <= 0.12.
#include "igt_launch.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace igt;

static const char* name(SearchKernel64 k) {
    switch (k) {
        case SearchKernel64::ORACLE: return "ORACLE";
        case SearchKernel64::LITERAL: return "LITERAL";
        case SearchKernel64::CAPTURE_STATIC: return "CAPTURE_STATIC";
        case SearchKernel64::CAPTURE_QUEUES: return "CAPTURE_QUEUES";
        case SearchKernel64::POOL: return "POOL";
        case SearchKernel64::UNITS_WAVES3: return "UNITS_WAVES3";
        case SearchKernel64::UNITS: return "UNITS";
        case SearchKernel64::CANDIDATES_STAGED: return "CANDIDATES_STAGED";
        case SearchKernel64::CANDIDATES_DIRECT: return "CANDIDATES_DIRECT";
    }
    return "?";
}
static const char* name(EmitKernel64 k) {
    switch (k) {
        case EmitKernel64::ORACLE: return "ORACLE";
        case EmitKernel64::GATHER: return "GATHER";
        case EmitKernel64::PIECES: return "PIECES";
        case EmitKernel64::ONE_PIECE: return "ONE_PIECE";
    }
    return "?";
}
static const char* name(SearchKernel32 k) {
    switch (k) {
        case SearchKernel32::WAVES3: return "WAVES3";
        case SearchKernel32::CHECKPOINTS: return "CHECKPOINTS";
        case SearchKernel32::TRACK: return "TRACK";
        case SearchKernel32::UNITS: return "UNITS";
    }
    return "?";
}
static const char* name(EmitKernel32 k) {
    switch (k) {
        case EmitKernel32::PIECES: return "PIECES";
        case EmitKernel32::ONE_PIECE: return "ONE_PIECE";
    }
    return "?";
}

static int bad(const char* item, const char* why) {
    std::fprintf(stderr, "handle_walk_plan: %s: %s\n", item, why);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return bad("usage", "handle_walk_plan <n_cu> <dtype,family,cost,N,C,B,concurrency,dev,own> ...");
    const int n_cu = std::atoi(argv[1]);
    if (n_cu < 1) return bad(argv[1], "n_cu must be positive");
    for (int i = 2; i < argc; ++i) {
        char dtype[8], family[16], cost[16];
        int N, C, B, conc, dev, own;
        if (std::sscanf(argv[i], "%7[^,],%15[^,],%15[^,],%d,%d,%d,%d,%d,%d", dtype, family, cost, &N, &C, &B, &conc, &dev, &own) != 9)
            return bad(argv[i], "nine comma-separated fields expected");
        const bool f64 = !std::strcmp(dtype, "f64");
        if (!f64 && std::strcmp(dtype, "f32")) return bad(argv[i], "dtype");
        const bool value = !std::strcmp(cost, "value_net");
        if (!value && std::strcmp(cost, "progress")) return bad(argv[i], "cost");
        KP P{};
        if (!std::strcmp(family, "lattice")) P.cand_mode = CAND_LATTICE;
        else if (!std::strcmp(family, "table")) P.cand_mode = CAND_TABLE;
        else if (!std::strcmp(family, "ramp_hold")) P.cand_mode = CAND_RAMP_HOLD;
        else if (!std::strcmp(family, "track")) P.cand_mode = CAND_TRACK;
        else return bad(argv[i], "family");
        if (N < 1 || C < 64 || C % 64 || B < 1 || conc < 1 || (own && (!f64 || P.cand_mode != CAND_TABLE))) return bad(argv[i], "range");
        P.N = N; P.C = C; P.n_rk4 = 4; P.cost_mode = value ? 1 : 0;
        P.hi_order = 0;                                                                    // restated: make_kp at the default limits
        P.G = P.cand_mode == CAND_TABLE ? 1 : (int)std::lround(std::sqrt((double)C));      // restated: make_kp
        P.dev = dev & DEV_ENV_MASK;
        const int waves_per_simd = conc >= 3 ? 1 : 2;                                      // restated: solve_impl
        std::printf("%s:", argv[i]);
        if (f64) {
            const Search64Plan p = own ? plan_candidates64(P, B, value)
                                       : plan_search64(P, B, value, Search64Env{n_cu, waves_per_simd, -1, -1, -1, false});
            std::printf(" search_kernel=%s emit_kernel=%s W=%d partials=%d grid=%zu queues=%d order_stride=%d live_rows=%d"
                        " rows_build_queues=%d rows_threads=%d separate_queue_builder=%d launch_dev_bits=%d seg_scenarios=%d"
                        " seg_lds_bytes=%zu traj_doubles=%zu ck_records=%zu queue_order_words=%zu memset_counters=%d"
                        " reset_rec_count=%d reset_best_key=%d emit_priority=%d ckpt_doubles=%zu\n",
                        name(p.search_kernel), name(p.emit_kernel), p.W, p.partials, p.grid, p.queues, p.order_stride,
                        (int)p.live_rows, (int)p.rows_build_queues, p.rows_threads, (int)p.separate_queue_builder, p.launch_dev_bits,
                        p.seg_scenarios, p.seg_lds_bytes, p.traj_doubles, p.ck_records, p.queue_order_words, (int)p.memset_counters,
                        (int)p.reset_rec_count, (int)p.reset_best_key, p.emit_priority, (size_t)p.ckpt_doubles);
        } else {
            const Search32Plan p = plan_search32(P, B, value, Search32Env{n_cu, waves_per_simd, -1, false});
            std::printf(" search_kernel=%s emit_kernel=%s W=%d partials=%d grid=%zu queues=%d order_stride=%d builds_queues=%d"
                        " launch_dev_bits=%d incumbents=%d ck_parts=%d emit_grid=%zu ckpt_doubles=%zu queue_order_words=%zu"
                        " memset_counters=%d reset_rec_count=%d reset_best_key=%d ck_records=%zu traj_doubles=%zu\n",
                        name(p.search_kernel), name(p.emit_kernel), p.W, p.partials, p.grid, p.queues, p.order_stride,
                        (int)p.builds_queues, p.launch_dev_bits, (int)p.incumbents(), p.ck_parts, p.emit_grid, p.ckpt_doubles,
                        p.queue_order_words, (int)p.memset_counters, (int)p.reset_rec_count, (int)p.reset_best_key,
                        (size_t)p.ck_records, (size_t)p.traj_doubles);
        }
    }
    return 0;
}
