// igt_dispatch.h -- the run-time fields of KP that choose a kernel build (cand_mode, hi_order, n_rk4 == 4), turned into
// template arguments in one place.  The launchers of igt_kernels_f64.hip and igt_kernels.hip go through with_family /
// with_discretisation; prepare_emit_kernels visits the same lists (for_each_*), so what it prepares is what they can launch.
// Plain C++17 without HIP types: a host compiler builds it alone (tests/dispatch_leaves.cpp).
#pragma once
#include <type_traits>

namespace igt {

enum { CAND_LATTICE = 0, CAND_TABLE = 1, CAND_RAMP_HOLD = 2, CAND_TRACK = 3 };

template <class... Leaf> struct Leaves {};

// The candidate families.  The last one is the fallback: every cand_mode the others do not claim, values outside the enum
// included, is a table of controls.
using Families = Leaves<std::integral_constant<int, CAND_LATTICE>, std::integral_constant<int, CAND_RAMP_HOLD>,
                        std::integral_constant<int, CAND_TRACK>, std::integral_constant<int, CAND_TABLE>>;

// The builds of one control step: HI = the long stage-offset polynomials (KP::hi_order); NRK = 4, the reference's four
// sub-steps unrolled with the short polynomials, or 0, any number of sub-steps at run time.  (HI, 4) does not exist: the
// long polynomials have the generic build only.
template <bool HI_, int NRK_>
struct Discretisation {
    static constexpr bool HI = HI_;
    static constexpr int NRK = NRK_;
};
using Discretisations = Leaves<Discretisation<true, 0>, Discretisation<false, 4>, Discretisation<false, 0>>;

// f(leaf) for the first leaf that matches, or for the last one
template <class Match, class F, class First, class... Rest>
auto with_first_leaf(Leaves<First, Rest...>, Match&& match, F&& f) {
    if constexpr (sizeof...(Rest) == 0) {
        return f(First{});
    } else {
        if (match(First{})) return f(First{});
        return with_first_leaf(Leaves<Rest...>{}, match, f);
    }
}
template <class F, class... Leaf>
void for_each_leaf(Leaves<Leaf...>, F&& f) {
    (f(Leaf{}), ...);
}

// f(std::bool_constant<flag>{})
template <class F>
auto with_bool(bool flag, F&& f) {
    if (flag) return f(std::true_type{});
    return f(std::false_type{});
}

// f(std::integral_constant<int, CAND>{}), once
template <class F>
auto with_cand(int cand_mode, F&& f) {
    return with_first_leaf(Families{}, [&](auto cand) { return cand_mode == cand(); }, f);
}
// f(std::integral_constant<int, CAND>{}, std::bool_constant<HI>{}), once: for the kernels without a build per number of sub-steps
template <class F>
auto with_family(int cand_mode, int hi_order, F&& f) {
    return with_cand(cand_mode, [&](auto cand) { return with_bool(hi_order != 0, [&](auto hi) { return f(cand, hi); }); });
}
// f(std::integral_constant<int, CAND>{}) for every family
template <class F>
void for_each_family(F&& f) {
    for_each_leaf(Families{}, f);
}

// f(std::bool_constant<HI>{}, std::integral_constant<int, NRK>{}), once
template <class F>
auto with_discretisation(int hi_order, int n_rk4, F&& f) {
    return with_first_leaf(
        Discretisations{},
        [&](auto d) { return decltype(d)::HI == (hi_order != 0) && (decltype(d)::NRK == 0 || decltype(d)::NRK == n_rk4); },
        [&](auto d) { return f(std::bool_constant<decltype(d)::HI>{}, std::integral_constant<int, decltype(d)::NRK>{}); });
}
// the same for every discretisation
template <class F>
void for_each_discretisation(F&& f) {
    for_each_leaf(Discretisations{},
                  [&](auto d) { f(std::bool_constant<decltype(d)::HI>{}, std::integral_constant<int, decltype(d)::NRK>{}); });
}

}  // namespace igt
