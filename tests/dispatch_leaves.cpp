// Stand-alone check of csrc/igt_dispatch.h and csrc/igt_roll_options.h (test_host_logic.py builds it with g++ -std=c++17 and the address / undefined-behaviour
// sanitizers and runs it): every (cand_mode, hi_order, n_rk4) reaches exactly one leaf, the expected one; what is no family is a
// table; (HI, 4) is never reached; the for_each_* lists visit 4 and 3 leaves, each once.
#include "igt_dispatch.h"
#include "igt_roll_options.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

using namespace igt;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

template <int CAND, bool HI>
struct FamilyLeaf {                    // what a launcher instantiates: the constants must be usable as template arguments
    static std::pair<int, bool> id() { return {CAND, HI}; }
};
template <bool HI, int NRK>
struct StepLeaf {
    static_assert(!(HI && NRK == 4), "(HI, 4) is no leaf");
    static std::pair<bool, int> id() { return {HI, NRK}; }
};

// csrc/igt_roll_options.h: the flags are distinct bits, and every role derives the LEAN and BOUND its call sites passed by
// position before the options had names.  The literals are those call sites': LEAN was BOOK && EARLY_EXIT, BOUND was
// CAND == CAND_TRACK && BOOK && UNIFORM && EARLY_EXIT (float32: && !SEG), with (BOOK, UNIFORM, EARLY_EXIT) = (true, true, true)
// at the search units, the capture and the pool, (false, false, false) at emit and its pieces, (true, true, false) at the
// polish and rollout-all, (false, true, false) at the literal mapping; the pool passed BOUND = false itself (lattice only).
constexpr unsigned ROLL_FLAGS[] = {ROLL_BOOK,       ROLL_UNIFORM, ROLL_EARLY_EXIT, ROLL_STEER_TABLE, ROLL_NO_XY,
                                   ROLL_LEAVE_CKPT, ROLL_RESUME,  ROLL_STEP_TABLE, ROLL_EY_FOLDED,   ROLL_PART_D};
constexpr bool distinct_bits() {
    unsigned seen = 0;
    for (unsigned f : ROLL_FLAGS) {
        if (f == 0 || (f & (f - 1)) != 0 || (seen & f) != 0) return false;
        seen |= f;
    }
    return true;
}
template <unsigned O>
constexpr bool derives(bool lean, bool bound_track) {
    return roll_supported(O) && roll_lean(O) == lean && roll_bound(CAND_TRACK, O) == bound_track && !roll_bound(CAND_LATTICE, O) &&
           !roll_bound(CAND_RAMP_HOLD, O) && !roll_bound(CAND_TABLE, O);
}
static_assert(distinct_bits(), "one bit per option");
static_assert(derives<ROLL_SEARCH>(true, true) && derives<ROLL_SEARCH | ROLL_STEER_TABLE>(true, true), "capture");
static_assert(derives<ROLL_SEARCH | ROLL_LEAVE_CKPT>(true, true) && derives<ROLL_SEARCH | ROLL_NO_XY>(true, true) &&
                  derives<ROLL_SEARCH | ROLL_LEAVE_CKPT | ROLL_STEER_TABLE | ROLL_NO_XY>(true, true), "search unit");
static_assert(roll_lean(ROLL_POOL | ROLL_STEP_TABLE) && roll_lean(ROLL_POOL | ROLL_LEAVE_CKPT | ROLL_NO_XY) &&
                  !roll_bound(CAND_LATTICE, ROLL_POOL | ROLL_STEP_TABLE) && !roll_bound(CAND_LATTICE, ROLL_POOL | ROLL_LEAVE_CKPT) &&
                  roll_supported(ROLL_POOL | ROLL_STEP_TABLE) && roll_supported(ROLL_POOL | ROLL_LEAVE_CKPT), "pool");
static_assert(derives<ROLL_EMIT>(false, false) && derives<ROLL_EMIT_PIECE>(false, false) &&
                  derives<ROLL_EMIT_PIECE | ROLL_NO_XY>(false, false), "emit, emit piece");
static_assert(derives<ROLL_POLISH>(false, false) && derives<ROLL_POLISH | ROLL_NO_XY>(false, false), "polish");
static_assert(derives<ROLL_ALL>(false, false) && derives<ROLL_LITERAL>(false, false), "rollout-all, literal");
static_assert(!roll_supported(ROLL_RESUME | ROLL_LEAVE_CKPT) && !roll_supported(ROLL_STEP_TABLE), "what no build uses");

int main() {
    const int cand_modes[] = {-1, 0, 1, 2, 3, 7}, hi_orders[] = {0, 1}, n_rk4s[] = {1, 2, 3, 4, 7};
    for (int cand_mode : cand_modes)
        for (int hi_order : hi_orders) {
            const bool family = cand_mode == CAND_LATTICE || cand_mode == CAND_RAMP_HOLD || cand_mode == CAND_TRACK;
            const int want = family ? cand_mode : CAND_TABLE;
            int calls = 0;
            const int ret = with_family(cand_mode, hi_order, [&](auto cand, auto hi) {
                ++calls;
                CHECK((FamilyLeaf<cand(), hi()>::id() == std::pair<int, bool>(want, hi_order != 0)));
                return 17;
            });
            CHECK(calls == 1 && ret == 17);
            calls = 0;
            with_cand(cand_mode, [&](auto cand) {
                ++calls;
                CHECK((FamilyLeaf<cand(), false>::id().first == want));
            });
            CHECK(calls == 1);
            for (int n_rk4 : n_rk4s) {
                calls = 0;
                with_discretisation(hi_order, n_rk4, [&](auto hi, auto nrk) {
                    ++calls;
                    const int want_nrk = !hi_order && n_rk4 == 4 ? 4 : 0;
                    CHECK((StepLeaf<hi(), nrk()>::id() == std::pair<bool, int>(hi_order != 0, want_nrk)));
                });
                CHECK(calls == 1);
            }
        }
    CHECK(CAND_LATTICE == 0 && CAND_TABLE == 1 && CAND_RAMP_HOLD == 2 && CAND_TRACK == 3);      // include/igtmpc.h IGT_CAND_*
    // hi_order is a flag: any non-zero value is the long polynomials
    with_discretisation(2, 4, [&](auto hi, auto nrk) { CHECK(hi() && nrk() == 0); });

    std::multiset<int> families;
    for_each_family([&](auto cand) { families.insert(cand()); });
    CHECK((families == std::multiset<int>{CAND_LATTICE, CAND_TABLE, CAND_RAMP_HOLD, CAND_TRACK}));
    std::multiset<std::pair<bool, int>> steps;
    for_each_discretisation([&](auto hi, auto nrk) { steps.insert(StepLeaf<hi(), nrk()>::id()); });
    CHECK((steps == std::multiset<std::pair<bool, int>>{{true, 0}, {false, 4}, {false, 0}}));

    for (bool flag : {false, true}) CHECK(with_bool(flag, [](auto b) { return (bool)b(); }) == flag);
    std::puts("dispatch leaves ok");
    return 0;
}
