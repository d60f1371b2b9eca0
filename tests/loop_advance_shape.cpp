// Stand-alone check of the launch shape of igt_loop_advance_* (csrc/igt_launch.h loop_grid, loop_block_agents, loop_walk;
// test_loop_advance_host.py builds the host side of it with the address / undefined-behaviour sanitizers and runs it): over
// n = 0..1000 agents and horizons N = 1..64, the workgroups the launcher starts, walked lane by lane the way
// loop_advance_kernel walks them, decide every agent exactly once and touch every element of x_sol's [n,7,N+1] and of u_sol's
// [n,2,N] exactly once, nothing outside.  The marks live in exactly-sized heap blocks, so a stray index is a sanitizer report.
#include "igt_launch.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

using namespace igt;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

constexpr int WORKERS = 8;      // the shapes are independent: worker w takes n = w, w + WORKERS, ...
std::atomic<long> shapes{0};

void check_shapes(int first) {
    for (int n = first; n <= 1000; n += WORKERS)
        for (int N = 1; N <= 64; ++N) {
            const size_t row_x = (size_t)7 * (N + 1), row_u = (size_t)2 * N;
            std::vector<unsigned char> agent((size_t)n, 0), ex((size_t)n * row_x, 0), eu((size_t)n * row_u, 0);
            const int grid = loop_grid(n);
            CHECK(grid == (n + LOOP_AGENTS - 1) / LOOP_AGENTS);
            for (int b = 0; b < grid; ++b) {
                const int agents = loop_block_agents(n, b);
                const size_t a0 = (size_t)b * LOOP_AGENTS;
                CHECK(agents >= 1 && agents <= LOOP_AGENTS && a0 + (size_t)agents <= (size_t)n);
                for (int t = 0; t < LOOP_THREADS; ++t) {
                    if (t < agents) ++agent.at(a0 + t);
                    loop_walk(agents, row_x, t, [&](size_t e) { ++ex.at(a0 * row_x + e); });
                    loop_walk(agents, row_u, t, [&](size_t e) { ++eu.at(a0 * row_u + e); });
                }
            }
            CHECK(loop_block_agents(n, grid) == 0);      // a workgroup past the grid would own nothing
            for (unsigned char c : agent) CHECK(c == 1);
            for (unsigned char c : ex) CHECK(c == 1);
            for (unsigned char c : eu) CHECK(c == 1);
            ++shapes;
        }
}

int main() {
    std::vector<std::thread> workers;
    for (int w = 0; w < WORKERS; ++w) workers.emplace_back(check_shapes, w);
    for (std::thread& t : workers) t.join();
    CHECK(LOOP_AGENTS <= LOOP_THREADS && LOOP_THREADS % 64 == 0);
    CHECK(loop_grid(-3) == 0 && loop_grid(2147483647) == 134217728);
    std::printf("loop advance shape ok: %ld shapes\n", shapes.load());
    return 0;
}
