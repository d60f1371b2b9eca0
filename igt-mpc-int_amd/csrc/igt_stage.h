// igt_stage.h -- where a host-mode call's buffers lie in the staging arena.  An entry point of igt_api.hip declares each buffer
// once (host pointer, bytes, direction, copied or only reserved); the offsets, the two spans that cross the bus and the 256 KiB
// packing rule follow from that list here, and nowhere else.  Plain C++17 without HIP types: a host compiler builds it alone
// (tests/stage_plan.cpp).
#pragma once
#include <cstddef>
#include <cstring>

namespace igt {

// A host-mode solve of a few scenarios is a dozen sub-kilobyte copies around ~120 us of kernels, and every pageable
// hipMemcpyAsync costs ~7 us whatever its size.  Up to PACK_BYTES the inputs are gathered into a pinned mirror of the
// staging arena and cross the bus in ONE copy, the outputs come back in one; beyond that the copies go directly (a second
// pass over megabytes on the host would cost more than the calls).
constexpr size_t PACK_BYTES = 256 * 1024;
constexpr size_t STAGE_ALIGN = 256;
constexpr int STAGE_MAX_BUFFERS = 16;      // the largest entry, a warm-started solve, has 13

struct StagePlan {
    struct Buf {
        void* host;        // the caller's array (an input's is only read)
        size_t bytes;      // reserved in the arena
        size_t off;        // set by layout()
        bool out, copy;
    };
    Buf buf[STAGE_MAX_BUFFERS];
    int n = 0;
    size_t in_span = 0;        // [0, in_span): the inputs
    size_t out_begin = 0;      // [out_begin, total): the outputs
    size_t total = 0;
    bool overflow = false;     // more than STAGE_MAX_BUFFERS were declared: the plan is unusable (Staging::upload refuses it)

    // One buffer of `bytes` bytes, `elem` each.  Returns its index, or -1 for an absent optional buffer: a null array that
    // would have been copied (a warm start, X_all / U_all, dV_out) takes no bytes at all.  A buffer that is not copied -- as
    // asked, or because it is empty (obs_xy at n_obs == 0) -- keeps a reservation of at least one element, so that the
    // kernels get a valid pointer.
    int add(const void* host, size_t bytes, size_t elem, bool out, bool copy = true) {
        copy = copy && bytes > 0;
        if (!host && copy) return -1;
        if (n == STAGE_MAX_BUFFERS) { overflow = true; return -1; }
        buf[n] = Buf{const_cast<void*>(host), bytes ? bytes : elem, 0, out, copy};
        return n++;
    }

    // 256-byte aligned offsets in the order of declaration, all inputs first and all outputs behind them: each group is one
    // contiguous span.
    void layout() {
        size_t off = 0;
        for (int pass = 0; pass < 2; ++pass) {
            bool first = true;
            for (int i = 0; i < n; ++i) {
                if (buf[i].out != (pass == 1)) continue;
                off = (off + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1);
                if (pass == 1 && first) out_begin = off;
                first = false;
                buf[i].off = off;
                off += buf[i].bytes;
            }
            if (pass == 0) in_span = out_begin = off;
        }
        total = off;
    }

    bool packed() const { return total <= PACK_BYTES; }

    // the packed path's two passes on the host: the copied inputs into a mirror of the arena, the copied outputs out of it
    void gather(void* mirror) const {
        for (int i = 0; i < n; ++i)
            if (!buf[i].out && buf[i].copy) std::memcpy(static_cast<char*>(mirror) + buf[i].off, buf[i].host, buf[i].bytes);
    }
    void scatter(const void* mirror) const {
        for (int i = 0; i < n; ++i)
            if (buf[i].out && buf[i].copy) std::memcpy(buf[i].host, static_cast<const char*>(mirror) + buf[i].off, buf[i].bytes);
    }
};

}  // namespace igt
