// Stand-alone check of the grid of the persistent float64 search (csrc/igt_launch.h search64_slots / search64_grid;
// test_search_grid_host.py builds the host side of it with the address / undefined-behaviour sanitizers and runs it): for
// n_cu in {1, 8, 256, 304}, one and two waves per SIMD, the reserve on and off (DEV_NO_RESERVE), both kernel families and
// every reserve a sweep may ask for -- the grid is never 0 and never above the slots, it is the slots below three solves in
// flight and with the switch, it never goes below one wave per queue while the chip has that many slots, and the slots -- the
// pools' batch bound is stated in them -- do not depend on the reserve or the switch.
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
    const int cus[] = {1, 8, 256, 304}, wps[] = {0, 1, 2}, per8s[] = {-1, 0, 1, 2, 4, 8, 31, 32, 33, 100000};
    const Search64 fams[] = {Search64::UNITS, Search64::POOL};
    const int others = DEV_NO_REFILL | DEV_NO_STEAL;             // switches that have nothing to do with the grid
    for (int n_cu : cus)
        for (int w : wps) {
            const size_t slots = (size_t)n_cu * 4 * (w == 1 ? 1 : 2);
            // the pools' bound B >= 4 * slots: the switch and the other bits leave the slots alone
            for (int dev : {0, (int)DEV_NO_RESERVE, others, others | (int)DEV_NO_RESERVE}) CHECK(search64_slots(n_cu, w, dev) == slots);
            const size_t floor = slots < (size_t)SEARCH64_QUEUES ? slots : (size_t)SEARCH64_QUEUES;
            for (Search64 f : fams) {
                size_t last = slots;
                for (int per8 : per8s) {
                    const size_t on = search64_grid(n_cu, w, f, others, per8), off = search64_grid(n_cu, w, f, others | DEV_NO_RESERVE, per8);
                    CHECK(off == slots);                                    // the switch: every slot
                    CHECK(on >= 1 && on <= slots && on >= floor);
                    if (w != 1) CHECK(on == slots);                         // below three solves in flight nothing changes
                    if (per8 == 0) CHECK(on == slots);
                    if (w == 1 && per8 > 0) {
                        const size_t reserve = (size_t)n_cu * (size_t)per8 / 8;
                        CHECK(on == (slots > reserve + floor ? slots - reserve : floor));
                        CHECK(on <= last);                                  // a larger reserve never gives a larger grid
                        last = on;
                    }
                    if (per8 == 100000) CHECK(w != 1 || on == floor);
                }
                // the shipped values (no override): what the default argument gives
                const int d = f == Search64::POOL ? SEARCH64_RESERVE_PER_8CU_POOL : SEARCH64_RESERVE_PER_8CU_UNITS;
                CHECK(search64_grid(n_cu, w, f, 0) == search64_grid(n_cu, w, f, 0, d));
            }
        }
    // the figures the write-up quotes
    CHECK(SEARCH64_QUEUES == 8 && search64_slots(256, 1, 0) == 1024 && search64_slots(256, 2, 0) == 2048);
    CHECK(4 * search64_slots(256, 1, DEV_NO_RESERVE) == 4096 && 4 * search64_slots(256, 1, 0) == 4096);   // B = 4096 takes the pools either way
    CHECK(search64_grid(256, 1, Search64::POOL, 0, 2) == 960 && search64_grid(304, 1, Search64::POOL, 0, 2) == 1140);
    CHECK(search64_grid(8, 1, Search64::POOL, 0, 2) == 30 && search64_grid(1, 1, Search64::POOL, 0, 2) == 4);
    CHECK(search64_grid(8, 1, Search64::POOL, 0, 32) == 8 && search64_grid(1, 1, Search64::POOL, 0, 32) == 4);
    CHECK(SEARCH64_RESERVE_PER_8CU_POOL >= 0 && SEARCH64_RESERVE_PER_8CU_POOL <= 8 && SEARCH64_RESERVE_PER_8CU_UNITS >= 0 &&
          SEARCH64_RESERVE_PER_8CU_UNITS <= 8);
    CHECK((DEV_NO_RESERVE & DEV_ENV_MASK) == DEV_NO_RESERVE);      // the environment may set it
    std::printf("search grid ok\n");
    return 0;
}
