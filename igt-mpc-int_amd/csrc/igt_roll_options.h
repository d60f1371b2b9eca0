// igt_roll_options.h -- the build options of a roll-out (igt_fast64.h rollout_one / rollout_pool and their step_head / step_tail /
// horizon_end; igt_fast_impl.inc rollout_pair) as one word of named flags, and what every build derives from it.
// Plain C++17 without HIP types: a host compiler builds it alone (tests/dispatch_leaves.cpp).
#pragma once
#include "igt_dispatch.h"

namespace igt {

enum RollOption : unsigned {
    ROLL_BOOK = 1u << 0,         // cost and verdicts are kept (off: emit, only the trajectory is produced)
    ROLL_UNIFORM = 1u << 1,      // the lanes of a wave roll one scenario (off: one scenario per lane, whole-step choices by votes)
    ROLL_EARLY_EXIT = 1u << 2,   // search: the wave stops once every candidate has failed; only "failed" is reported then
    ROLL_STEER_TABLE = 1u << 3,  // steering column (lattice, ramp-hold) or control sequence (table family) read from stab
    ROLL_NO_XY = 1u << 4,        // x, y are neither integrated nor judged (obstacles out of reach; emit pieces)
    ROLL_LEAVE_CKPT = 1u << 5,   // search: leaves the horizon checkpoints a roll-out resumes from (ck / Ckpt)
    ROLL_RESUME = 1u << 6,       // emit in pieces: rolls steps [seg_k0, seg_k1) from such a record (ck / Seg)
    ROLL_STEP_TABLE = 1u << 7,   // pool: the column is fill_pool_table's -- sblr and the rotation by beta_k - beta_k-1 come from it
    ROLL_EY_FOLDED = 1u << 8,    // pool: |ey_k| - ey_lim is in gmax already when step_head books state k
    ROLL_PART_D = 1u << 9,       // pool: a whole step taken as K == 0 leaves d0, d1 alone (Fast64::substeps WHOLE_D = false)
    ROLL_BOX = 1u << 10,         // the collision verdict is the rectangle (OBCA) one: S.obs is fill_box_table's table, not [n_obs,2,N+1]
};
// The roles.  A call adds what its site decides on top: ROLL_STEER_TABLE, ROLL_NO_XY, ROLL_LEAVE_CKPT / ROLL_STEP_TABLE.
constexpr unsigned ROLL_SEARCH = ROLL_BOOK | ROLL_UNIFORM | ROLL_EARLY_EXIT;                    // search unit, capture
constexpr unsigned ROLL_POOL = ROLL_SEARCH | ROLL_STEER_TABLE | ROLL_EY_FOLDED | ROLL_PART_D;   // rollout_pool
constexpr unsigned ROLL_ALL = ROLL_BOOK | ROLL_UNIFORM;                                         // rollout-all
constexpr unsigned ROLL_POLISH = ROLL_ALL | ROLL_STEER_TABLE;                                   // trial plans of the polish
constexpr unsigned ROLL_EMIT = 0u;                                                              // the winner, one scenario per lane
constexpr unsigned ROLL_EMIT_PIECE = ROLL_RESUME;                                               // one piece of it
constexpr unsigned ROLL_LITERAL = ROLL_UNIFORM;                                                 // north_star's literal mapping

// LEAN: search only needs feasible-or-not -- |ey|, box v and collision are folded into one running maximum gmax, compared with
// the tolerance when it is read (x > tol for some x  <=>  max x > tol; a NaN operand is ignored by both forms).
constexpr bool roll_lean(unsigned o) { return (o & ROLL_BOOK) && (o & ROLL_EARLY_EXIT); }
// BOUND: the incumbent bound (igt_fast64.h) -- the tracking family's search, whose candidates hardly ever fail a verdict.
constexpr bool roll_bound(int cand, unsigned o) {
    return cand == CAND_TRACK && (o & ROLL_SEARCH) == ROLL_SEARCH && !(o & ROLL_RESUME);
}
// what no build uses and the code does not support
constexpr bool roll_supported(unsigned o) {
    return !((o & ROLL_RESUME) && (o & ROLL_LEAVE_CKPT)) && !((o & ROLL_STEP_TABLE) && !(o & ROLL_STEER_TABLE)) &&
           !((o & ROLL_BOX) && (o & ROLL_STEP_TABLE));      // the rectangle verdict reads (sin, cos)(beta_k-1), which the pool's lanes do not carry
}

}  // namespace igt
