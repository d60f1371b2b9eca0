// Stand-alone check of csrc/igt_dispatch.h (test_host_logic.py builds it with g++ -std=c++17 and the address / undefined-behaviour
// sanitizers and runs it): every (cand_mode, hi_order, n_rk4) reaches exactly one leaf, the expected one; what is no family is a
// table; (HI, 4) is never reached; the for_each_* lists visit 4 and 3 leaves, each once.
#include "igt_dispatch.h"

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
