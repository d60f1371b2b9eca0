// igt_value_polish_layout.h -- where the polish under the value-network cost (igt_set_value_polish; igt_kernels_f64.hip
// value_trials_f64_kernel / value_accept_f64_kernel) keeps its scratch in a solve's workspace.  The host takes doubles(B, N) of
// the workspace in solve_impl's one carve and hands the kernels the base; host and kernels find every piece from the base
// through this one declaration.  Offsets are in doubles from the base (256-byte aligned by the carve); every piece starts on an
// even offset, that is 16-byte aligned.  Plain C++17 without HIP types, every function constexpr: a host compiler builds it alone
// (tests/value_polish_layout.cpp) and device code calls it as it is.
#pragma once
#include <cstddef>

namespace igt {

constexpr int VALUE_POLISH_TRIALS = 64;          // trials per scenario and iteration: one per lane of the scenario's wave
constexpr int VALUE_POLISH_MAX_ITERS = 4;
constexpr int VN_DOUBLES_PER_SCENARIO = 5;       // igt_launch.h VnScratch: (s_N, v_N), V, (dV/ds_N, dV/dv_N)
// the largest batch the polish takes: the network launch over the trials counts 64 B rows, and two words each, in int
constexpr int VALUE_POLISH_MAX_B = 0x7fffffff / (2 * VALUE_POLISH_TRIALS);

struct ValuePolishLayout {
    size_t B, N;
    constexpr ValuePolishLayout(int B_, int N_) : B((size_t)B_), N((size_t)N_) {}
    static constexpr size_t even(size_t n) { return (n + 1) & ~(size_t)1; }
    constexpr size_t rows() const { return B * VALUE_POLISH_TRIALS; }       // trial records: row b 64 + m
    // per scenario
    constexpr size_t grad() const { return 0; }                              // [B, 2, N] dJ/du at the plan
    constexpr size_t grad_cost() const { return grad() + even(B * 2 * N); }  // [B] the gradient sweep's own cost (not read)
    constexpr size_t vn() const { return grad_cost() + even(B); }            // VnScratch of the gradient's three launches
    // per trial
    constexpr size_t stage() const { return vn() + even(VN_DOUBLES_PER_SCENARIO * B); }      // [rows] stage cost
    constexpr size_t feas() const { return stage() + even(rows()); }         // [rows] uint32 verdict bits (0: feasible)
    constexpr size_t sv() const { return feas() + even((rows() + 1) / 2); }  // [rows, 2] (s_N, v_N)
    constexpr size_t tv_sv() const { return sv() + even(rows() * 2); }       // [rows, 2] the scenario's tv_sv
    constexpr size_t enc() const { return tv_sv() + even(rows() * 2); }      // [rows, 2] the scenario's enc
    constexpr size_t V() const { return enc() + even(rows() * 2); }          // [rows] the network's values
    // per scenario
    constexpr size_t alive() const { return V() + even(rows()); }            // [B] int32: still polished
    constexpr size_t doubles() const { return alive() + even((B + 1) / 2); }
    static constexpr size_t doubles(int B_, int N_) { return ValuePolishLayout(B_, N_).doubles(); }
};

}  // namespace igt
