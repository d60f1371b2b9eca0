// Stand-alone check of csrc/igt_value_polish_layout.h (test_value_polish_layout_host.py builds it with g++ -std=c++17 and the
// address / undefined-behaviour sanitizers and runs it): for B in {1, 17, 64, 300, 65 536} x N in {1, 20, 64} the pieces are
// 16-byte aligned, hold what the kernels keep in them, do not overlap and lie inside doubles(B, N); every word of every piece is
// written once into an exactly-sized heap block (the sanitizer sees an overrun); and at B = 65 536 no count the launches form in
// int -- the 64 B trial rows, their two words each, B 2 N -- passes INT_MAX.
#include "igt_value_polish_layout.h"

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace igt;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

struct Piece {
    const char* name;
    size_t off;        // doubles from the base
    size_t bytes;      // what the kernels keep there
};

void check(int B, int N, bool touch) {
    const ValuePolishLayout L(B, N);
    const size_t b = (size_t)B, n = (size_t)N, rows = b * 64;
    CHECK(L.rows() == rows && VALUE_POLISH_TRIALS == 64);
    const Piece pc[] = {
        {"grad", L.grad(), b * 2 * n * 8},       {"grad_cost", L.grad_cost(), b * 8}, {"vn", L.vn(), b * 5 * 8},
        {"stage", L.stage(), rows * 8},          {"feas", L.feas(), rows * 4},        {"sv", L.sv(), rows * 16},
        {"tv_sv", L.tv_sv(), rows * 16},         {"enc", L.enc(), rows * 16},         {"V", L.V(), rows * 8},
        {"alive", L.alive(), b * 4},
    };
    const int np = (int)(sizeof(pc) / sizeof(pc[0]));
    const size_t total = ValuePolishLayout::doubles(B, N);
    CHECK(total == L.doubles() && total % 2 == 0);
    size_t sum = 0;
    for (int i = 0; i < np; ++i) {
        CHECK(pc[i].off % 2 == 0);                                   // 16 bytes
        CHECK(pc[i].bytes > 0 && pc[i].off * 8 + pc[i].bytes <= total * 8);
        for (int j = 0; j < np; ++j)
            if (j != i) CHECK(pc[i].off * 8 + pc[i].bytes <= pc[j].off * 8 || pc[j].off * 8 + pc[j].bytes <= pc[i].off * 8);
        sum += pc[i].bytes;
    }
    CHECK(total * 8 < sum + (size_t)np * 16);                        // no more than the padding of each piece
    // what the launches count in int
    CHECK(rows <= (size_t)INT_MAX && rows * 2 <= (size_t)INT_MAX && b * 2 * n <= (size_t)INT_MAX && total <= (size_t)INT_MAX);
    CHECK(B <= VALUE_POLISH_MAX_B);
    if (!touch) return;
    std::unique_ptr<unsigned char[]> blk(new unsigned char[total * 8]());
    for (int i = 0; i < np; ++i)
        for (size_t k = 0; k < pc[i].bytes; ++k) {
            CHECK(blk[pc[i].off * 8 + k] == 0);                      // nobody else's
            blk[pc[i].off * 8 + k] = (unsigned char)(i + 1);
        }
}

int main() {
    const int Bs[] = {1, 17, 64, 300, 65536}, Ns[] = {1, 20, 64};
    for (int B : Bs)
        for (int N : Ns) check(B, N, B <= 300);
    CHECK((long long)VALUE_POLISH_MAX_B * 2 * VALUE_POLISH_TRIALS <= (long long)INT_MAX);
    CHECK(VN_DOUBLES_PER_SCENARIO == 5 && VALUE_POLISH_MAX_ITERS == 4);
    std::printf("value polish layout ok\n");
    return 0;
}
