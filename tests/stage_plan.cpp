// Stand-alone check of csrc/igt_stage.h (test_host_logic.py builds it with g++ -std=c++17 and the address / undefined-behaviour
// sanitizers and runs it): offsets are multiples of 256, buffers do not overlap, inputs lie below in_span and outputs in
// [out_begin, total); an absent optional buffer takes no bytes, a reserved one keeps an element and is not moved; the totals
// of one solve worked out by hand; the 256 KiB rule; gather / scatter on exactly-sized heap blocks.
#include "igt_stage.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace igt;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// an exactly-sized heap block (no slack for an overrun to hide in), filled with a pattern of its own
struct Block {
    std::unique_ptr<unsigned char[]> p;
    size_t n;
    Block(size_t bytes, unsigned seed) : p(bytes ? new unsigned char[bytes] : nullptr), n(bytes) {
        for (size_t i = 0; i < n; ++i) p[i] = (unsigned char)(seed * 37 + i * 11 + 1);
    }
    bool equals(const Block& o) const { return n == o.n && (n == 0 || std::memcmp(p.get(), o.p.get(), n) == 0); }
};

// the properties every laid-out plan has
void check_layout(const StagePlan& pl) {
    CHECK(pl.in_span <= pl.out_begin && pl.out_begin <= pl.total && pl.out_begin % 256 == 0);
    for (int i = 0; i < pl.n; ++i) {
        const StagePlan::Buf& b = pl.buf[i];
        CHECK(b.off % 256 == 0 && b.bytes > 0);
        if (b.out) CHECK(b.off >= pl.out_begin && b.off + b.bytes <= pl.total);
        else CHECK(b.off + b.bytes <= pl.in_span);
        for (int j = 0; j < i; ++j) {
            const StagePlan::Buf& c = pl.buf[j];
            CHECK(b.off + b.bytes <= c.off || c.off + c.bytes <= b.off);
        }
    }
}

// The buffers of solve_impl<double> (csrc/igt_api.hip) for B scenarios, horizon N, n_obs obstacles, progress cost: tv_sv / enc
// are reserved and not copied.  `arr` holds the host blocks in the order of declaration (null: an absent warm start).
struct Solve {
    std::vector<Block> arr;
    StagePlan pl;
    int i_tv, i_ws;
    Solve(size_t B, size_t N, size_t n_obs, bool warm) {
        const size_t in_bytes[] = {B * 7 * 8, B * 2 * 8, B * 3 * 8, B * 4, B * n_obs * 2 * (N + 1) * 8, B * 2 * 8, B * 2 * 8,
                                   B * 2 * N * 8};
        const size_t out_bytes[] = {B * 7 * (N + 1) * 8, B * 2 * N * 8, B * 8, B * 4, B * 4};
        unsigned seed = 0;
        for (size_t b : in_bytes) arr.emplace_back(b, ++seed);
        for (size_t b : out_bytes) arr.emplace_back(b, ++seed);
        for (int k = 0; k < 5; ++k) CHECK(pl.add(arr[k].p.get(), arr[k].n, k == 3 ? 4 : 8, false) == k);
        i_tv = pl.add(arr[5].p.get(), arr[5].n, 8, false, false);
        CHECK(pl.add(arr[6].p.get(), arr[6].n, 8, false, false) == 6);
        i_ws = pl.add(warm ? arr[7].p.get() : nullptr, arr[7].n, 8, false);
        for (int k = 8; k < 13; ++k) CHECK(pl.add(arr[k].p.get(), arr[k].n, k >= 11 ? 4 : 8, true) >= 0);
        pl.layout();
    }
};

int main() {
    {   // float64, B = 3, N = 20, n_obs = 1, no warm start.  By hand, each offset the previous end rounded up to 256:
        //   x0 168 B at 0, u_prev 48 at 256, kparams 72 at 512, flags 12 at 768, obs_xy 1008 at 1024, tv_sv 48 at 2048,
        //   enc 48 at 2304 -> in_span 2352; x_out 3528 at 2560, u_out 960 at 6144 (6088 rounded up), cost 24 at 7168,
        //   argmin 12 at 7424, status 12 at 7680 -> total 7692
        Solve s(3, 20, 1, false);
        check_layout(s.pl);
        CHECK(s.i_ws == -1 && s.pl.n == 12);
        CHECK(s.pl.in_span == 2352 && s.pl.out_begin == 2560 && s.pl.total == 7692 && s.pl.packed());
        const size_t off[] = {0, 256, 512, 768, 1024, 2048, 2304, 2560, 6144, 7168, 7424, 7680};
        for (int i = 0; i < 12; ++i) CHECK(s.pl.buf[i].off == off[i]);
    }
    {   // the same with a warm start: u_ws 960 at 2560 -> in_span 3520; x_out at 3584 ends 7112, u_out at 7168 ends 8128,
        // cost at 8192, argmin at 8448, status 12 at 8704 -> total 8716
        Solve s(3, 20, 1, true);
        check_layout(s.pl);
        CHECK(s.i_ws == 7 && s.pl.n == 13);
        CHECK(s.pl.in_span == 3520 && s.pl.out_begin == 3584 && s.pl.total == 8716);

        // gather / scatter through a mirror of exactly `total` bytes
        Block mirror(s.pl.total, 99), before(s.pl.total, 99);
        s.pl.gather(mirror.p.get());
        for (int i = 0; i < s.pl.n; ++i) {
            const StagePlan::Buf& b = s.pl.buf[i];
            if (b.out) continue;
            const unsigned char* want = b.copy ? (const unsigned char*)b.host : before.p.get() + b.off;      // reserved: not moved
            CHECK(std::memcmp(mirror.p.get() + b.off, want, b.bytes) == 0);
        }
        CHECK(!s.pl.buf[s.i_tv].copy && s.pl.buf[s.i_tv].bytes == 48);
        CHECK(std::memcmp(mirror.p.get() + s.pl.in_span, before.p.get() + s.pl.in_span, s.pl.total - s.pl.in_span) == 0);
        // as the kernels would: every output written in the mirror, then scattered into the caller's arrays
        for (size_t i = s.pl.out_begin; i < s.pl.total; ++i) mirror.p[i] = (unsigned char)(i * 7 + 3);
        std::vector<Block> inputs;
        for (int k = 0; k < 8; ++k) inputs.emplace_back(s.arr[k].n, k + 1);
        s.pl.scatter(mirror.p.get());
        for (int i = 0; i < s.pl.n; ++i) {
            const StagePlan::Buf& b = s.pl.buf[i];
            if (b.out) CHECK(std::memcmp(b.host, mirror.p.get() + b.off, b.bytes) == 0);
        }
        for (int k = 0; k < 8; ++k) CHECK(s.arr[k].equals(inputs[k]));      // scatter leaves the inputs alone
    }
    {   // round trip: what gather put into the mirror, scatter gives back unchanged
        Block src(1000, 1), dst(1000, 2), src2(3, 3), dst2(3, 4);
        StagePlan pl;
        pl.add(src.p.get(), 1000, 8, false); pl.add(src2.p.get(), 3, 1, false);
        pl.add(dst.p.get(), 1000, 8, true); pl.add(dst2.p.get(), 3, 1, true);
        pl.layout();
        check_layout(pl);
        CHECK(pl.in_span == 1027 && pl.out_begin == 1280 && pl.total == 2307);
        Block mirror(pl.total, 5);
        pl.gather(mirror.p.get());
        std::memcpy(mirror.p.get() + pl.buf[2].off, mirror.p.get() + pl.buf[0].off, 1000);      // a kernel that copies
        std::memcpy(mirror.p.get() + pl.buf[3].off, mirror.p.get() + pl.buf[1].off, 3);
        pl.scatter(mirror.p.get());
        CHECK(dst.equals(src) && dst2.equals(src2));
    }
    {   // reserved and absent buffers; declaration order need not be inputs first
        double x[4] = {1, 2, 3, 4}, y[4];
        StagePlan pl;
        CHECK(pl.add(y, sizeof y, 8, true) == 0);
        CHECK(pl.add(nullptr, 0, 8, false) == 1);                 // empty (obs_xy at n_obs == 0, null or not): one element kept
        CHECK(pl.add(x, 0, 4, false) == 2);
        CHECK(pl.add(nullptr, 64, 8, false, false) == 3);         // not copied (plans absent): reserved as declared
        CHECK(pl.add(nullptr, 64, 8, true) == -1);                // optional output not wanted
        CHECK(pl.add(nullptr, 64, 8, false) == -1);               // optional input not given
        CHECK(pl.add(x, sizeof x, 8, false) == 4 && pl.n == 5);
        pl.layout();
        check_layout(pl);
        CHECK(pl.buf[1].bytes == 8 && pl.buf[2].bytes == 4 && pl.buf[3].bytes == 64);
        CHECK(!pl.buf[1].copy && !pl.buf[2].copy && !pl.buf[3].copy && pl.buf[4].copy);
        CHECK(pl.buf[1].off == 0 && pl.buf[2].off == 256 && pl.buf[3].off == 512 && pl.buf[4].off == 768);
        CHECK(pl.in_span == 800 && pl.out_begin == 1024 && pl.buf[0].off == 1024 && pl.total == 1056);
        Block mirror(pl.total, 7), before(pl.total, 7);
        pl.gather(mirror.p.get());                                // a null or empty reserved buffer is never read
        CHECK(std::memcmp(mirror.p.get(), before.p.get(), 768) == 0 && std::memcmp(mirror.p.get() + 768, x, 32) == 0);
    }
    for (size_t extra : {0, 1}) {   // the packing rule: at most 256 KiB
        StagePlan pl;
        unsigned char one = 0;
        pl.add(&one, 1, 1, false);
        pl.add(&one, 262144 - 256 + extra, 1, true);              // (laid out only: never copied here)
        pl.layout();
        CHECK(pl.total == 262144 + extra && pl.packed() == (extra == 0));
    }
    {   // one buffer too many: refused, nothing written past the list, and the plan says so
        StagePlan pl;
        unsigned char one = 0;
        for (int i = 0; i < STAGE_MAX_BUFFERS; ++i) CHECK(pl.add(&one, 1, 1, i % 2 == 1) == i && !pl.overflow);
        CHECK(pl.add(&one, 1, 1, true) == -1 && pl.overflow && pl.n == STAGE_MAX_BUFFERS);
    }
    CHECK(PACK_BYTES == 262144 && STAGE_MAX_BUFFERS >= 13);
    std::puts("stage plan ok");
    return 0;
}
