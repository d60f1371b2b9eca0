/*
 * igtmpc.h -- C ABI of the MI355X-native batched MPC rollout + shooting solver.
 *
 * The reference (hansungkim98122/IGT-MPC-INT) is pure Python and has NO FFI for
 * this path: its boundary is the Python object API that evaluate.py consumes
 * (MPC_Planner.update_initial_condition / update_predictions / solve,
 * mpc.py:241-294, 383-406).  Each entry point below therefore cites the
 * reference lines whose work it replaces; INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, caller-allocated buffers.
 *   - every function returns 0 on success, <0 on error (IGT_E_*); the message is
 *     available from igt_last_error() (thread-local).  Nothing throws.
 *   - `mem` says where the caller's buffers live: IGT_MEM_DEVICE (HBM pointers,
 *     work is enqueued on `stream` and the call returns without synchronising)
 *     or IGT_MEM_HOST (the library stages through its own device buffers and
 *     synchronises before returning).
 *   - `stream` is a hipStream_t passed as void* (NULL = the handle's own non-blocking stream; pass
 *     hipStreamLegacy, (void*)1, to name the legacy default stream).
 *   - state order everywhere: [x, y, s, ey, epsi, v, psi]      (mpc.py:163)
 *   - array layouts are C-contiguous with the shapes written in the comments.
 *   - one handle per (device, thread); handles share no mutable state.  A handle owns its workspace: two solves
 *     on one handle must not overlap in time (use one handle per stream).
 *   - IGT_MEM_DEVICE calls only enqueue work (kernels and memset nodes; no allocation once the workspace has its
 *     size, no host synchronisation), so after one warm-up call a solve can be captured in a stream graph.
 */
#ifndef IGTMPC_H
#define IGTMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGT_VERSION 201

enum {
    IGT_OK = 0,
    IGT_E_INVALID = -1,   /* bad argument / unsupported parameter combination */
    IGT_E_HIP = -2,       /* a HIP runtime call failed                        */
    IGT_E_NOMEM = -3,
    IGT_E_STATE = -4      /* e.g. value-net cost requested but no net loaded  */
};

enum { IGT_MEM_DEVICE = 0, IGT_MEM_HOST = 1 };

/* candidate control-sequence families (build-defined: the reference's NLP has no
 * candidates; SURVEY.md section 8d defines the lattice used for the benchmark) */
enum {
    IGT_CAND_LATTICE = 0,  /* G x G lattice of constant per-step (da, ddf) increments */
    IGT_CAND_TABLE = 1,    /* explicit table U[C,2,N] shared by every scenario         */
    IGT_CAND_RAMP_HOLD = 2,/* G x G: a and df track, at the rate limits, base sequence + one of G offsets each; the
                              base is u_prev held over the horizon or -- igt_solve_batch_ws_* -- the warm start (the
                              previous solution shifted by one step); offsets are dense around 0 (first pass) and, with
                              refine_iters > 0, re-centred on the previous pass's winner with its grid cell's spacing */
    IGT_CAND_TRACK = 3     /* G x G: acceleration as IGT_CAND_RAMP_HOLD (offset i from the base sequence) with the target
                              kept under the envelope E_k = track_env dt^2 (N - k - 1/2) / (2 w_u) -- the acceleration
                              beyond which one more unit costs more effort (mpc.py:362) than it buys progress
                              (mpc.py:372); STEERING is a
                              state feedback evaluated inside the roll-out: beta_cmd = clamp(-epsi - track_ke * ey + off_j),
                              df tracks atan(tan(beta_cmd) (l_f + l_r) / l_r) at the steering-rate limit.  Every
                              acceleration profile thereby gets the steering that belongs to where it actually is;
                              the realised (a_k, df_k) are returned as u_out like any other candidate's            */
};

/* cost (mpc.py:356-373) */
enum {
    IGT_COST_PROGRESS = 0, /* ... - (s_N - s_0)                 eval_mode mpc,    mpc.py:372 */
    IGT_COST_VALUE_NET = 1 /* ... - (V(Wn(x_N-mu))*sig + mu_t)  eval_mode gt_mpc, mpc.py:369 */
};

/* per-scenario flag bits (flags[B]) */
#define IGT_FLAG_ABS_HEADING 1u /* ego route in {'32','41'}: psi_0 = |psi_0|  (mpc.py:231-234, 282-285) */
#define IGT_FLAG_WARM 2u        /* the scenario's row of u_ws holds a warm start (igt_solve_batch_ws_*)          */

/* violation bits reported by igt_rollout_batch_* (viol_out) */
#define IGT_VIOL_BOX_V 1u      /* mpc.py:316-317  k = 0..N-1 */
#define IGT_VIOL_BOX_U 2u      /* mpc.py:318-321            */
#define IGT_VIOL_RATE 4u       /* mpc.py:301-312  (table candidates only; lattices satisfy it by construction) */
#define IGT_VIOL_EY 8u         /* mpc.py:296-299  k = 0..N   */
#define IGT_VIOL_TERMINAL 16u  /* mpc.py:177-180  C_inf * [v_{N-1}; a_{N-1}] <= b */
#define IGT_VIOL_COLLISION 32u /* mpc.py:223-226  k = 1..N   */
#define IGT_VIOL_NONFINITE 64u /* a non-finite state (|.| >= 1e300 counts) or a non-finite cost */

#define IGT_MAX_N 64
#define IGT_MAX_CINF 256
#define IGT_MAX_OBS 4

typedef struct igt_handle igt_handle;

/* The constants MPC_Planner.__init__ hard-codes (mpc.py:45-62) plus the
 * discretisation (N, dt, n_rk4) and the candidate family.
 * igt_create refuses (IGT_E_INVALID) anything outside these ranges: every double
 * below is finite; dt, l_r, l_f > 0; v_min <= v_max; a_min <= a_max;
 * 0 <= df_max < pi/2 (the steering model takes tan(df)); jerk_limit > 0;
 * steer_rate_limit >= 0; feas_tol >= 0. */
typedef struct igt_params {
    int32_t N;         /* horizon                      (mpc.py:38; evaluate.py:69)  */
    int32_t n_rk4;     /* RK4 sub-steps per control step (evaluate.py:109 -> 4)     */
    int32_t C;         /* candidates per solve; multiple of 64; lattices need C = G*G */
    int32_t n_obs;     /* obstacles per scenario = M-1  (mpc.py:83)                 */
    int32_t cand_mode; /* IGT_CAND_*  */
    int32_t cost_mode; /* IGT_COST_*  */
    double dt;         /* fourwayint.yaml:2  */
    double l_r, l_f;   /* mpc.py:49-50       */
    double v_min, v_max, a_min, a_max, df_max; /* mpc.py:57-62; v_min <= v_max, a_min <= a_max, 0 <= df_max < pi/2 */
    double jerk_limit;       /* mpc.py:56; > 0 */
    double steer_rate_limit; /* mpc.py:55; >= 0 */
    double ey_lim;           /* mpc.py:61 */
    double d_min;            /* 2*ca_radius, mpc.py:45 */
    double w_u;              /* 0.05, mpc.py:362 */
    double feas_tol;         /* inequality verdicts are g <= feas_tol; >= 0 */
    int32_t refine_iters;    /* IGT_CAND_RAMP_HOLD / IGT_CAND_TRACK: extra search passes around the winner (0..4) */
    int32_t polish_iters;    /* _f64, IGT_COST_PROGRESS: projected-gradient steps on the winner after the search (0..4);
                                0 = the best candidate as it is.  See igt_solve_batch_*                                   */
    double track_ke;         /* IGT_CAND_TRACK: lateral-error gain of the steering feedback [1/m]          (0.3)  */
    double track_span;       /* IGT_CAND_TRACK: the G slip-angle offsets span +-track_span [rad]            (0.1)  */
    double track_beta_lim;   /* IGT_CAND_TRACK: |beta_cmd| limit [rad]                                      (0.7)  */
    double track_env;        /* IGT_CAND_TRACK: scale of the acceleration envelope E_k; 0 = no envelope     (1.0)
                                Applied with IGT_COST_PROGRESS only: E_k is derived from the progress term
                                (mpc.py:372), which the IGT_COST_VALUE_NET cost does not have (mpc.py:367-370) */
    double track_vcap;       /* IGT_CAND_TRACK: > 0: the acceleration targets also stay under the speed cap -- the largest
                                a_k from which a jerk-limited ramp to a = 0 (mpc.py:301-304) still keeps v <= v_max
                                (mpc.py:316-317): a candidate with a large offset accelerates at the limits and arrives
                                at v_max with a = 0 instead of failing the speed box; 0 = off: no cap at all  (1.0)  */
} igt_params;

/* Fills *p with the reference's numbers: N=20, dt=0.1, n_rk4=4, C=256, n_obs=1,
 * lattice candidates, progress cost, mpc.py:45-62 limits, feas_tol=1e-6. */
int igt_params_default(igt_params* p);

const char* igt_last_error(void);
int igt_version(void);

/* Replaces MPC_Planner.__init__ (mpc.py:21-160) for a whole batch: no NLP is
 * built; the handle owns a stream, staging buffers and the constant tables. */
int igt_create(const igt_params* p, int device, igt_handle** out);
int igt_destroy(igt_handle* h);
int igt_get_params(const igt_handle* h, igt_params* out);

/* Terminal set C_inf as half-planes A[F,2] * (v, a) <= b[F]
 * (mpc.py:88-104 builds it with polytope; 177-180 applies it). F = 0 disables. */
int igt_set_cinf(igt_handle* h, const double* A, const double* b, int32_t F);

/* Explicit candidate table U[C,2,N] (row 0 = a_k, row 1 = df_k) for IGT_CAND_TABLE. */
int igt_set_candidate_table(igt_handle* h, const double* U);

/* Terminal value network (mpc.py:108-127, 367-369; model.py:14-51).
 * n_layers Linear layers, dims[n_layers+1] = {6,128,...,1}; weights holds, per
 * layer, W[out,in] row-major followed by b[out].  Wn[6,6], mu_f[6]: input
 * whitening x -> Wn (x - mu_f); sigma_t, mu_t: target de-normalisation. */
int igt_set_value_net(igt_handle* h, int32_t n_layers, const int32_t* dims, const double* weights,
                      const double* Wn, const double* mu_f, double sigma_t, double mu_t);

/* The batched solve.  Replaces, per scenario b, one
 *   update_initial_condition (mpc.py:280-294) + update_predictions (241-278) + solve (383-406)
 * of the reference by: generate C candidate control sequences from u_prev[b],
 * roll each through the RK4 Frenet bicycle model
 * (kinematic_bicycle_model_frenet.py:70-127 == mpc.py:201-209), evaluate the cost
 * (mpc.py:356-373) and every constraint (mpc.py:177-180, 223-226, 296-321), and
 * return the feasible arg-min (ties -> lowest candidate index).
 *
 *   x0      [B,7]              initial state                       (mpc.py:280-292)
 *                              Angles: psi_0 = x0[6] and epsi_0 = x0[4] are reduced by the library's own two-term
 *                              Cody-Waite reduction; the solve is accurate (the bars below) for |psi_0|, |epsi_0| <= 1e6,
 *                              any multiple of 2 pi included.  Beyond 1e6 -- NaN and inf included -- the scenario is
 *                              answered status 1, never status 0 with non-finite rows.
 *   u_prev  [B,2]              previously applied (a, df)          (mpc.py:286)
 *   kparams [B,3]              curvature (b0, b1, Kv): K(s) = Kv [s >= b0] - Kv [s >= b1] (mpc.py:183-200 pw_const), i.e.
 *                              Kv on [b0,b1) else 0 for b0 <= b1; straight routes pass (inf, inf, 0).  Any other values
 *                              mean what the formula says: a NaN break-point is never reached, b1 < b0 gives -Kv on
 *                              [b1,b0), and a non-finite Kv makes every state from b0 on non-finite.
 *   flags   [B]                IGT_FLAG_*
 *   obs_xy  [B,n_obs,2,N+1]    obstacle x / y predictions, already passed through
 *                              filter_preds (utils.py:365-388); k = 1..N are read, obs_xy[..., 0] is not.  A non-finite
 *                              coordinate never collides: that node of that obstacle is no constraint (NaN, +-inf),
 *                              the nodes beside it stay what they are.
 *   tv_sv   [B,2]  enc [B,2]   value-net cost only (may be NULL otherwise):
 *                              (s,v) of the other vehicle's last raw prediction and
 *                              (e_ego, e_tv) scenario encodings     (mpc.py:326-338)
 *   x_out   [B,7,N+1]  u_out [B,2,N]   arg-min trajectory / controls (mpc.py:401)
 *   cost_out[B]  argmin_out[B]  status_out[B]
 *        status 0 <-> is_opt True; 1 <-> no feasible candidate (is_opt False,
 *        mpc.py:402-406): then argmin = -1, cost = +inf, x_out/u_out = NaN.
 *        A candidate with a non-finite state or cost is infeasible, so a scenario whose inputs leave none finite -- a
 *        non-finite x0, a NaN in u_prev or in a warm start that is read (an infinite one is clamped to the input box), a
 *        non-finite tv_sv / enc under the value-network cost -- is answered status 1, and no scenario's answer depends on another scenario's inputs.
 *
 * polish_iters > 0 (_f64 entries, IGT_COST_PROGRESS; igt_create refuses it with IGT_COST_VALUE_NET, the _f32 entries
 *       answer IGT_E_INVALID): after the search every solved scenario's winner is improved on the device by up to
 *       polish_iters steps of: forward-difference gradient of the cost over the 2 N inputs (eps = 1e-4), 64 trial steps
 *       u + 2^(-m/3) d along d = -gradient scaled so that the longest moves some input by four rate limits, every trial
 *       clamped step by step to the rate window and the input box and judged by all verdicts; the cheapest feasible trial
 *       is taken when it is strictly cheaper, else the scenario stops.  x_out, u_out, cost_out are then those of the
 *       polished plan (x_out its roll-out, the bits igt_rollout_batch_f64 gives for u_out as a table candidate; cost_out
 *       never above the winner's); argmin_out stays the index of the candidate the polish STARTED from -- u_out is no
 *       longer that candidate's controls; status_out and unsolved scenarios are untouched.  No host synchronisation, no
 *       extra workspace: such a solve is captured in a stream graph and overlapped like any other.
 *
 * _f64: double everywhere -- the reference's precision.  The RK4 stages are evaluated in factorised form
 *       (csrc/igt_fast64.h); <= 1e-9 of the float64 oracle on every trajectory (measured ~1e-14).
 * _f32: float storage, float stage derivatives, double state accumulators; within 1e-5*max(1,|ref|) of the
 *       float64 oracle except where a curvature switch is decided inside float32 noise.
 */
int igt_solve_batch_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev,
                        const float* kparams, const uint32_t* flags, const float* obs_xy,
                        const float* tv_sv, const float* enc, float* x_out, float* u_out,
                        float* cost_out, int32_t* argmin_out, int32_t* status_out, int mem,
                        void* stream);
int igt_solve_batch_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev,
                        const double* kparams, const uint32_t* flags, const double* obs_xy,
                        const double* tv_sv, const double* enc, double* x_out, double* u_out,
                        double* cost_out, int32_t* argmin_out, int32_t* status_out, int mem,
                        void* stream);

/* The same solve with a warm start -- what the reference passes to solve(x_sol_prev, u_sol_prev) after
 * augment_prev_sol (utils.py:354-363; call site evaluate.py:478-482): the previous solution's controls shifted by one
 * step and extended by repeating the last one.  IPOPT starts its iterations there; the shooting solver centres its
 * candidate set there: IGT_CAND_RAMP_HOLD targets become u_ws[b,:,k] + offset (instead of u_prev + offset), so the
 * shifted previous plan is itself candidate (G/2, G/2).  The state part x_sol_prev has no counterpart (shooting states
 * are implied by the controls).
 *   u_ws [B,2,N]   rows are read only where flags[b] & IGT_FLAG_WARM; NULL = no warm start anywhere.
 * Needs cand_mode IGT_CAND_RAMP_HOLD or IGT_CAND_TRACK (acceleration base only) when u_ws != NULL. */
int igt_solve_batch_ws_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev,
                           const float* kparams, const uint32_t* flags, const float* obs_xy,
                           const float* tv_sv, const float* enc, const float* u_ws, float* x_out,
                           float* u_out, float* cost_out, int32_t* argmin_out, int32_t* status_out,
                           int mem, void* stream);
int igt_solve_batch_ws_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev,
                           const double* kparams, const uint32_t* flags, const double* obs_xy,
                           const double* tv_sv, const double* enc, const double* u_ws, double* x_out,
                           double* u_out, double* cost_out, int32_t* argmin_out, int32_t* status_out,
                           int mem, void* stream);

/* Debug / parity entry: every candidate of every scenario.
 *   X_all [B,C,7,N+1] (may be NULL)   U_all [B,C,2,N] (may be NULL)
 *   cost_all [B,C]   viol_all [B,C] (IGT_VIOL_* bits; 0 = feasible) */
int igt_rollout_batch_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev,
                          const float* kparams, const uint32_t* flags, const float* obs_xy,
                          const float* tv_sv, const float* enc, float* X_all, float* U_all,
                          float* cost_all, uint32_t* viol_all, int mem, void* stream);
int igt_rollout_batch_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev,
                          const double* kparams, const uint32_t* flags, const double* obs_xy,
                          const double* tv_sv, const double* enc, double* X_all, double* U_all,
                          double* cost_all, uint32_t* viol_all, int mem, void* stream);

int igt_rollout_batch_ws_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev,
                             const float* kparams, const uint32_t* flags, const float* obs_xy,
                             const float* tv_sv, const float* enc, const float* u_ws, float* X_all,
                             float* U_all, float* cost_all, uint32_t* viol_all, int mem, void* stream);
int igt_rollout_batch_ws_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev,
                             const double* kparams, const uint32_t* flags, const double* obs_xy,
                             const double* tv_sv, const double* enc, const double* u_ws, double* X_all,
                             double* U_all, double* cost_all, uint32_t* viol_all, int mem, void* stream);

/* One control step of the RK4 Frenet bicycle model for n independent states -- the model
 * object the reference's driver calls directly for warm-start extension and for the
 * brake fallback (kinematic_bicycle_model_frenet.py:16-192 numpy branch; call sites
 * utils.py:358, evaluate.py:520).  Uses the handle's dt, n_rk4, l_r, l_f.
 *   x [n,7]   u [n,2] = (a, df)   kparams [n,3]   x_next [n,7]
 * _f64 follows the reference operation for operation (<= 1e-12 of the golden transitions).  _f32 uses the float
 * arithmetic of the solver with its long stage-offset polynomials: within 1e-5*max(1,|ref|) for |v| <= 25 m/s. */
int igt_frenet_step_f32(igt_handle* h, int32_t n, const float* x, const float* u, const float* kparams,
                        float* x_next, int mem, void* stream);
int igt_frenet_step_f64(igt_handle* h, int32_t n, const double* x, const double* u, const double* kparams,
                        double* x_next, int mem, void* stream);

/* ---- opponent forecast on the device ------------------------------
 * Route geometry for igt_forecast_batch_*: n_routes x 12 doubles per route
 *   (p0x, p0y, tx, ty, cx, cy, b0, b1, R, endx, endy, straight)
 * = start point of s, unit tangent, side the arc bends to, arc interval [b0,b1], radius, the frozen end
 * coordinates the reference uses after the arc, straight flag (utils.py:532-586 frenet2global, table-driven). */
int igt_set_routes(igt_handle* h, int32_t n_routes, const double* table);

/* What each ego planner is told about its opponent at a timestep, for B problems at once.  Replaces
 * ConstantAccelerationModel.predict (constant_acceleration_model.py:18-82), share_motion_forecasts
 * (utils.py:339-352: an opponent that solved last step shares its plan, shifted by one step and extended by
 * one predicted step; a = 0 if that step would exceed v = 5) and filter_preds (utils.py:365-388: an opponent
 * behind the ego is moved to (-20,-20)).  Scenes of M = n_obs + 1 vehicles (mpc.py:82-83 is written for any M; the shipped
 * fourwayint.yaml has M = 2): every per-opponent array carries an n_obs axis behind B, the opponents of a scene are forecast,
 * shared and filtered independently (with n_obs = 1 the shapes are the two-vehicle ones, [B,4], [B], ...).
 *   ego_xyh  [B,3]  ego x, y, heading                opp [B,n_obs,4]  opponent x, y, s, v (current)
 *   opp_a    [B,n_obs]  opponent's last applied a    opp_route [B,n_obs]  route id (row of the igt_set_routes table)
 *   plan_x [B,n_obs,7,N+1], plan_u [B,n_obs,2,N], has_plan [B,n_obs] (int32, 0 = no shared plan)  -- all three may be NULL
 *   obs_xy [B,n_obs,2,N+1] (out)   tv_sv [B,n_obs,2] (out): (s, v) of every opponent's last forecast state (mpc.py:263-276; the
 *   value network's features read the one of a two-vehicle scene, mpc.py:330) */
int igt_forecast_batch_f32(igt_handle* h, int32_t B, const float* ego_xyh, const float* opp, const float* opp_a,
                           const int32_t* opp_route, const float* plan_x, const float* plan_u,
                           const int32_t* has_plan, float* obs_xy, float* tv_sv, int mem, void* stream);
int igt_forecast_batch_f64(igt_handle* h, int32_t B, const double* ego_xyh, const double* opp, const double* opp_a,
                           const int32_t* opp_route, const double* plan_x, const double* plan_u,
                           const int32_t* has_plan, double* obs_xy, double* tv_sv, int mem, void* stream);

/* The same forecast for E whole scenes, scene-major: one row per AGENT, nothing gathered.  M = n_obs + 1 agents per scene
 * (2 .. IGT_MAX_OBS + 1); problem e M + i is agent i of scene e as ego, and its opponents are the agents j != i of the scene
 * in ascending j -- the order filter_preds(preds, i) leaves (utils.py:365-388); with M = 2 "the other one".  Every agent is
 * forecast (or its shared plan shifted) ONCE per scene and filtered per ego; the outputs are what igt_solve_batch_* reads for
 * the E M problems and equal igt_forecast_batch_* on the gathered inputs bit for bit (same device arithmetic).
 *   x [E,M,7] planner state order          a_prev [E,M] last applied a          route [E,M] row of the igt_set_routes table
 *   plan_x [E,M,7,N+1], plan_u [E,M,2,N], has_plan [E,M] (int32, 0 = no shared plan)  -- all three may be NULL
 *   obs_xy [E M,n_obs,2,N+1] (out)         tv_sv [E M,n_obs,2] (out)
 * IGT_MEM_DEVICE: one kernel enqueued on `stream`, no allocation, no host synchronisation (capturable).  IGT_E_INVALID for
 * E < 0, a handle without routes or with n_obs = 0.  (Added without a change of IGT_VERSION: nothing existing changed; a
 * caller that must run against an older library probes the symbol.) */
int igt_forecast_scene_f32(igt_handle* h, int32_t E, const float* x, const float* a_prev, const int32_t* route,
                           const float* plan_x, const float* plan_u, const int32_t* has_plan, float* obs_xy, float* tv_sv,
                           int mem, void* stream);
int igt_forecast_scene_f64(igt_handle* h, int32_t E, const double* x, const double* a_prev, const int32_t* route,
                           const double* plan_x, const double* plan_u, const int32_t* has_plan, double* obs_xy, double* tv_sv,
                           int mem, void* stream);

/* ---- pose forecast: the obstacles' x, y AND heading, what igt_solve_batch_box_f64 reads ------------------------------
 * Route headings for the pose entries below, a table of its own beside igt_set_routes (whose 12-double layout does not move):
 * n_routes x 3 doubles per route, (h0, hN, abs) = the heading before the arc, the heading after it, and whether this route's
 * headings are read as |heading| (non-zero: routes '32' and '41', mpc.py:250-253).  IGT_E_INVALID, with a message that names
 * the cause, for a null handle or table, a handle without routes, n_routes different from the igt_set_routes table's, a
 * non-finite h0 / hN.  A later igt_set_routes with another n_routes drops the headings. */
int igt_set_route_headings(igt_handle* h, int32_t n_routes, const double* table);

/* igt_forecast_scene_f64 with obs_pose [E M,n_obs,3,N+1] in place of obs_xy.  Rows 0 and 1 (x, y) and tv_sv are what
 * igt_forecast_scene_f64 writes for the same inputs, bit for bit ((-20, -20) behind an ego included).  Row 2 is the heading of
 * agent j's forecast as the reference's 'obca' ego reads it (utils.py:339-352, constant_acceleration_model.py:46-74); with s_k
 * the forecast's own arc length at node k:
 *   no shared plan   node 0: the true heading x[e,j,6]; node k >= 1: psi_ref(route, s_k);
 *   shared plan      node k < N: plan_x[e,j,6,k+1]; node N: psi_ref(route, s_ext), s_ext one predicted step behind the plan's
 *                    end (with the retry a = 0 above v = 5, as for x, y);
 *   psi_ref(r, s)    h0 on a straight route, else h0 + w (hN - h0), w = (s - b0) / (b1 - b0) clamped to [0, 1];
 *   abs flag set     the absolute value of all of the above.
 * The heading is NOT filtered: an agent behind an ego keeps its heading row while its x, y become -20.  Where s is not finite, x
 * and y are not finite either (the box verdict drops such a node) and the heading there is unspecified.
 * IGT_MEM_DEVICE: one kernel enqueued on `stream`, no allocation, no host synchronisation (capturable).  IGT_E_INVALID where
 * igt_forecast_scene_f64 says so, and for a handle without igt_set_route_headings.  _f64 only: the box solve has no float32
 * entry.  (Added without a change of IGT_VERSION; callers probe the symbols.) */
int igt_forecast_scene_pose_f64(igt_handle* h, int32_t E, const double* x, const double* a_prev, const int32_t* route,
                                const double* plan_x, const double* plan_u, const int32_t* has_plan, double* obs_pose,
                                double* tv_sv, int mem, void* stream);

/* The per-problem counterpart: igt_forecast_batch_f64 plus opp_heading [B,n_obs], every opponent's true heading (node 0 without a
 * shared plan), and obs_pose [B,n_obs,3,N+1] in place of obs_xy.  Same rules; igt_forecast_scene_pose_f64 equals this entry on
 * the gathered inputs bit for bit. */
int igt_forecast_batch_pose_f64(igt_handle* h, int32_t B, const double* ego_xyh, const double* opp, const double* opp_a,
                                const int32_t* opp_route, const double* opp_heading, const double* plan_x, const double* plan_u,
                                const int32_t* has_plan, double* obs_pose, double* tv_sv, int mem, void* stream);

/* 4-state Cartesian forward-Euler bicycle (kinematic_bicycle_model.py:15-50), the
 * model ReferenceGen.py steps to lay out reference paths.
 *   z0 [n,4] = (x, y, psi, v)   u [n,2,T] (a, df)   z_out [n,4,T+1] */
int igt_cartesian_euler_f32(igt_handle* h, int32_t n, int32_t T, const float* z0, const float* u,
                            float* z_out, int mem, void* stream);
int igt_cartesian_euler_f64(igt_handle* h, int32_t n, int32_t T, const double* z0, const double* u,
                            double* z_out, int mem, void* stream);

/* ---- multi-GPU: the one exchange of the path ---------------------------------------------------
 * Scenarios are independent (evaluate.py:469-558: the agents of a timestep solve against the same predictions), so a
 * batch shards into contiguous blocks, one process and one handle per GPU, with NO collective on the data path.  The
 * only exchange is an all-gather of the first-step controls u*[:, :, 0] -- the (a, df) every agent applies
 * (evaluate.py:492) -- so that each rank holds the whole action vector.  RCCL (ncclAllGather over xGMI) is bound at run
 * time with dlopen: a single-GPU user needs no RCCL, and a host that already carries one (torch ships librccl.so.1,
 * and `torch.distributed` is how bench.py and igtmpc/sharding.py do the same exchange) is not given a second copy.
 *   igt_comm_unique_id : rank 0 creates the 128-byte id; the caller distributes it (MPI_Bcast, a file, a socket).
 *   igt_comm_init      : every rank, same id; one communicator per handle.
 *   igt_allgather_controls_* : u_out [B_local,2,N] (device) -> u0_all [world*B_local,2] (device), rank-major, enqueued
 *                        on `stream`.  Equal shards (ncclAllGather); ragged shards are padded by the caller: with a
 *                        communicator EVERY rank must call with the same B_local > 0 -- an empty shard or a size
 *                        that differs from the communicator's first call returns IGT_E_INVALID instead of leaving the
 *                        peers waiting inside the collective.  Without a communicator (world = 1) it reduces to the
 *                        strided copy u0_all = u_out[:, :, 0] (B_local = 0: nothing to do). */
#define IGT_COMM_ID_BYTES 128
int igt_comm_unique_id(void* id_out /* IGT_COMM_ID_BYTES */);
int igt_comm_init(igt_handle* h, int32_t world, int32_t rank, const void* id);
int igt_comm_destroy(igt_handle* h);
int igt_allgather_controls_f32(igt_handle* h, int32_t B_local, const float* u_out, float* u0_all, void* stream);
int igt_allgather_controls_f64(igt_handle* h, int32_t B_local, const double* u_out, double* u0_all, void* stream);

/* How many solves the caller keeps in flight on this device at a time -- on other handles and streams -- including this
 * handle's (default 1).  The search kernels are persistent: with 1 a kernel starts as many waves as the device holds, two per
 * SIMD, which is fastest for a solve that has the device to itself.  When solves overlap, a second kernel only gets wave
 * slots as the first one drains, and a slot that has been vacated stays idle for tens of microseconds before the next
 * workgroup runs there; with `solves_in_flight` >= 3 a search kernel takes one wave per SIMD, so that two kernels are
 * resident side by side and each one's waves run faster while the other's are being replaced (measured at B = 4096 with four
 * solves in flight: 0.187 -> 0.176 ms per step; one solve alone: 0.277 -> 0.324, hence a setting and not the default; with
 * two in flight the streams of this runtime end up on one hardware queue and run one after the other, so 2 is treated as 1).
 * From 3 on, the float64 emit pass also stays one lean kernel (one wave per 64 scenarios, no LDS) instead of the five-wave,
 * LDS-staged emit in pieces that a solve with the device to itself uses to cut the winner roll-out's latency: between two
 * persistent search kernels only the lean one gets on the chip.  From 3 on, the float64 lattice's pool search also leaves one wave
 * slot in 32 untaken (32 of 1024 at 256 compute units; measured with four solves in flight: +4 % on the step rate, with three: -1.3 %).
 * Results do not depend on it.  IGT_E_INVALID unless 1 <= solves_in_flight <= 64. */
int igt_set_concurrency(igt_handle* h, int32_t solves_in_flight);

/* Which gradient the polish of the winner takes its direction from (polish_iters > 0; default IGT_GRAD_FORWARD_DIFF: the 2 N
 * forward differences described at igt_solve_batch_*, today's launch sequence and bits).  IGT_GRAD_ADJOINT: the analytic
 * gradient of the cost at the current plan -- the derivative igt_cost_gradient_f64 returns -- from the plan's node states and one
 * costate sweep; direction scaling, the 64 projected trials judged by every verdict and acceptance only when strictly cheaper
 * are unchanged, and so is everything the polish promises about x_out, u_out, cost_out, argmin_out, status_out, workspace and
 * stream capture.  The two gradients differ by the forward difference's truncation (order 1e-4 J''), so the polished plans are
 * close, not equal.  A setter and not a member of igt_params: that struct is not versioned.  IGT_E_INVALID for any other mode.
 * (Added without a change of IGT_VERSION; a caller that must run against an older library probes the symbol.) */
enum { IGT_GRAD_FORWARD_DIFF = 0, IGT_GRAD_ADJOINT = 1 };
int igt_set_polish_gradient(igt_handle* h, int mode);

/* Which step the polish of the winner tries (polish_iters > 0; default IGT_POLISH_STEP_GRADIENT: the 64 trials along the scaled
 * negative gradient, the launch sequence and bits of a handle that never called this).  IGT_POLISH_STEP_NEWTON adds the
 * Gauss-Newton (LQ, iLQR) direction from the Jacobians the analytic gradient is made of.  Per solved scenario and iteration, from
 * the plan u [2, N] with node states x_k and cost J0:
 *   1. T_k (3 x 5): rows (s, ey, epsi) of x_k+1 by (ey, epsi, v) of x_k and by (a_k, df_k), K(s) locally constant, and the
 *      analytic gradient g by the costate recursion (non-finite entries 0) -- IGT_GRAD_ADJOINT's, whatever
 *      igt_set_polish_gradient says; that setting is kept and applies again when the step is set back.
 *   2. LQ model over z = (ey, epsi, v):  A_k = T_k rows 1-2, columns 0-2, over the row (0, 0, 1);  B_k = T_k rows 1-2, columns
 *      3-4, over the row (dt, 0);  Q = diag(2, 2, 0),  R = 2 w_u I.  The s row enters the linear terms only (the costate of s
 *      is -1 throughout):  q_k = (2 ey_k, 2 epsi_k, 0) - T_k[0, 0:3],  r_k = 2 w_u u_k - T_k[0, 3:5].  The cost is a sum of
 *      squares plus a linear term, so the model is exact in the cost; only the curvature of the dynamics is dropped.
 *   3. Riccati sweep from P_N = Q, p_N = (2 ey_N, 2 epsi_N, 0), k = N-1 .. 0:  Quu = R + B'PB,  Qux = B'PA,  Qu = r + B'p,
 *      K = -Quu^-1 Qux,  kappa = -Quu^-1 Qu (the 2 x 2 inverse by the determinant formula),  P <- Q + A'PA + Qux'K,
 *      symmetrised (the upper triangle mirrored),  p <- q + A'p + Qux'kappa.
 *   4. Forward sweep:  dz_0 = 0,  dN_k = kappa_k + K_k dz_k,  dz_k+1 = A_k dz_k + B_k dN_k.  Non-finite entries of dN become 0;
 *      a determinant that is non-finite or <= 0 makes the whole dN of that scenario and iteration 0; with steer_rate = 0 the
 *      steering row is 0, as for the gradient direction.  dN is not rescaled: trial 0 is the full Newton step.
 *   5. Trials: lane m < 32 is project(u + 2^(-m/3) dN), lane m >= 32 is project(u + 2^(-(m-32)/3) dG) with dG the scaled -g of
 *      the gradient step (four rate limits on the longest trial).  Projection, verdicts, the cheapest feasible trial with ties
 *      to the lowest m and acceptance only when strictly cheaper are the gradient step's.
 * Everything the polish promises holds as written at igt_solve_batch_*: x_out is u_out's own table roll-out bit for bit, the
 * cost never rises, argmin_out, status_out and unsolved scenarios are untouched, no workspace, capturable.  The refusals of
 * polish_iters are unchanged (value-network cost, _f32, developer kernels).  A setter for the reason given above.
 * IGT_E_INVALID for a null handle or a mode that is neither IGT_POLISH_STEP_ constant.  (Added without a change of
 * IGT_VERSION; a caller that must run against an older library probes the symbol.) */
enum { IGT_POLISH_STEP_GRADIENT = 0, IGT_POLISH_STEP_NEWTON = 1 };
int igt_set_polish_step(igt_handle* h, int mode);

/* Polish of the winner under the value-network cost (IGT_COST_VALUE_NET, the _f64 solve entries; default 0: the launch sequence and
 * bits of a handle that never called this).  With iters = k in 1..4 a solve enqueues, behind the emit pass and on its own
 * stream, k iterations on every solved scenario's plan u [2, N] with cost J0 = stage terms - V_out(s_N, v_N) (mpc.py:356-369):
 *   1. g = dJ/du at the plan, as igt_cost_gradient_vn_f64 returns it; non-finite entries become 0;
 *   2. d = -g / scale, scale = max(max|g_a| / (4 dt jerk), max|g_df| / (4 dt steer_rate)) + 1e-30 (steer_rate = 0: the steering
 *      row of d is 0 and its term is left out);
 *   3. 64 trials u + 2^(-m/3) d, clamped step by step to the rate window around the clamped step before it, then to the box;
 *      each is rolled and judged by every verdict (the rate verdict included) and priced stage terms - V_out of its own
 *      terminal state;
 *   4. the feasible trial of least cost, ties to the lowest m, is accepted only if strictly cheaper than J0; else the scenario
 *      stops for good.
 * x_out is u_out's own table roll-out bit for bit, cost_out never rises, argmin_out, status_out and unsolved scenarios are
 * untouched.  Six launches an iteration whatever the batch, none sized by a count read from the device, no host
 * synchronisation; IGT_MEM_HOST and IGT_MEM_DEVICE alike.  The scratch (64 trial records per scenario) is part of the solve's
 * workspace, which therefore grows on the first eager solve after the call.
 * Stream capture is refused while iters > 0: a solve on a capturing stream returns IGT_E_STATE ("stream capture") before it
 * stages or enqueues anything.  An earlier build of this loop ended in an illegal memory access when replayed from a stream
 * graph and the cause was not found; until it is, capture a solve with iters = 0.
 * polish_iters, the progress cost's polish, keeps refusing the value network.  The _f32 solve entries and the developer kernels
 * of IGT_DEV_FLAGS 1024 / 2048 refuse a handle with iters > 0 (IGT_E_INVALID).
 * IGT_E_INVALID for a null handle, iters outside 0..4, or a handle whose cost is not IGT_COST_VALUE_NET.  (Added without a change
 * of IGT_VERSION; a caller that must run against an older library probes the symbol.) */
int igt_set_value_polish(igt_handle* h, int iters);

/* dJ/du of the progress cost for one control sequence per scenario:
 *   J(u) = sum_{k<=N} (epsi_k^2 + ey_k^2) + w_u sum_{k<N} (a_k^2 + df_k^2) - (s_N - s_0)            (mpc.py:356-373)
 * over the RK4 Frenet roll-out from x0 with the handle's dt, n_rk4, l_r, l_f, differentiated by every a_k and df_k.  No
 * projection, no verdicts: limits, obstacles and the terminal set play no part.  K(s) is taken as locally constant, which is
 * the derivative wherever no RK stage argument sits on a curvature break-point.
 *   x0 [B,7]  kparams [B,3]  flags [B]  U [B,2,N]  ->  cost_out [B]  grad_out [B,2,N]
 * flags are accepted as a solve's are (IGT_FLAG_ABS_HEADING acts on psi_0, which the cost does not read).  A non-finite cost
 * gives that scenario a NaN gradient row.  cost_out agrees with igt_rollout_batch_f64's cost of the same controls to rounding
 * (~1e-12), not bit for bit.  IGT_MEM_DEVICE: one kernel enqueued on `stream`, no workspace, no allocation, no host
 * synchronisation (capturable).  IGT_E_INVALID on a handle with IGT_COST_VALUE_NET, for B < 0 and for null buffers; B = 0 is a
 * no-op.  (Added without a change of IGT_VERSION; callers probe the symbol.) */
int igt_cost_gradient_f64(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags,
                          const double* U, double* cost_out, double* grad_out, int mem, void* stream);

/* The terminal term of the gt_mpc cost and its partials, for n terminal ego states of their own scenarios:
 *   V_out[i] = V(Wn (x_N - mu_f)) * sigma_t + mu_t,   x_N = [s_tv, v_tv, e_tv, s_N - s_tv, v_N - v_tv, e_ego - e_tv]
 * -- the amount mpc.py:369 subtracts from the cost -- with the network, whitening and scaling of igt_set_value_net, and
 *   dV_out[i] = (dV_out/ds_N, dV_out/dv_N)
 * by two forward-mode tangents through the same layers (only features 3 and 4 depend on the plan, mpc.py:326-338).
 *   sv [n,2] = (s_N, v_N)  tv_sv [n,2]  enc [n,2] = (e_ego, e_tv)  ->  V_out [n]  dV_out [n,2] (may be NULL: values alone, same bits)
 * float64 matrix cores on the weight fragments the solve uses; agrees with the value inside igt_rollout_batch_f64's cost to
 * rounding (~1e-13), not bit for bit.  A non-finite input gives that state NaN outputs.  IGT_MEM_DEVICE: one kernel enqueued on
 * `stream`, no workspace, no allocation, no host synchronisation (capturable).  IGT_E_INVALID on a handle that is not
 * IGT_COST_VALUE_NET, for n < 0, for null buffers (dV_out excepted) and for a bad mem; IGT_E_STATE when no network is loaded;
 * n = 0 is a no-op.  There is no _f32 entry.  (Added without a change of IGT_VERSION; callers probe the symbol.) */
int igt_terminal_value_f64(igt_handle* h, int32_t n, const double* sv, const double* tv_sv, const double* enc,
                           double* V_out, double* dV_out, int mem, void* stream);

/* dJ/du of the value-network cost (gt_mpc) for one control sequence per scenario:
 *   J(u) = sum_{k<=N} (epsi_k^2 + ey_k^2) + w_u sum_{k<N} (a_k^2 + df_k^2) - V_out(s_N, v_N)         (mpc.py:356-369)
 * with V_out as igt_terminal_value_f64 defines it.  Shapes and conventions are igt_cost_gradient_f64's -- no projection, no
 * verdicts, K(s) locally constant, a non-finite cost gives a NaN row, IGT_FLAG_ABS_HEADING accepted and inert -- plus the
 * scenario's tv_sv [B,2] and enc [B,2] as a solve takes them:
 *   x0 [B,7]  kparams [B,3]  flags [B]  tv_sv [B,2]  enc [B,2]  U [B,2,N]  ->  cost_out [B]  grad_out [B,2,N]
 * The costate starts at (-dV_out/ds_N, 2 ey_N, 2 epsi_N, -dV_out/dv_N); v_N = v_0 + dt sum a_k carries the last entry to
 * every a_k.  cost_out agrees with igt_rollout_batch_f64's cost of the same controls on a value-network handle to rounding.
 * Three kernels (forward sweep, network, forward and backward sweep) and 40 B of workspace per scenario, which grows as a
 * solve's does (below).  IGT_MEM_DEVICE: after one call at that B the call only enqueues kernels on `stream` -- no allocation,
 * no host synchronisation (capturable); growth under capture returns IGT_E_STATE.  IGT_E_INVALID on a handle that is not
 * IGT_COST_VALUE_NET (igt_cost_gradient_f64 keeps refusing those), for B < 0, for null buffers and for a bad mem; IGT_E_STATE
 * when no network is loaded; B = 0 is a no-op.  There is no _f32 entry.  (Added without a change of IGT_VERSION; callers
 * probe the symbol.) */
int igt_cost_gradient_vn_f64(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags,
                             const double* tv_sv, const double* enc, const double* U, double* cost_out, double* grad_out,
                             int mem, void* stream);

/* Per-scenario candidate sets: solve, and roll out all, on U [B,C,2,N] -- scenario b's C control sequences (a_k, then df_k, as
 * igt_set_candidate_table lays one table out), read from wherever the other buffers of the call live.  For every scenario b the
 * answer is what igt_solve_batch_f64 / igt_rollout_batch_f64 give for that scenario on a handle of the same parameters whose
 * shared table is U[b], bit for bit: ties go to the lowest index, status 1 carries NaN rows, +inf and -1, the rate limit and the
 * input box are judged as for any table candidate, a row of U with a NaN makes that candidate infeasible, and no scenario's
 * answer depends on another scenario's inputs, U among them.  Every other buffer, both costs (IGT_COST_VALUE_NET: tv_sv / enc
 * and a loaded network), polish_iters and igt_set_value_polish are igt_solve_batch_f64's / igt_rollout_batch_f64's.
 * The handle must be IGT_CAND_TABLE, which fixes C and N; igt_set_candidate_table need not have been called.
 * U follows `mem` like the other buffers.  IGT_MEM_HOST: it is staged with them, 16 C N bytes per scenario (82 KB at C = 256,
 * N = 20: a host-mode call pays for that copy).  IGT_MEM_DEVICE: the call only enqueues; after one call at that B it neither
 * allocates nor synchronises (capturable), and a replayed graph reads what U holds at replay time.
 * IGT_E_INVALID for a null handle, B < 0, a null U, a handle of another candidate family and with the developer kernels of
 * IGT_DEV_FLAGS 1024 / 2048; B = 0 is a no-op.  There is no _f32 entry: the float kernels read a double table and would need a
 * conversion pass of their own.  (Added without a change of IGT_VERSION; callers probe the symbols.) */
int igt_solve_candidates_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                             const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc,
                             const double* U, double* x_out, double* u_out, double* cost_out, int32_t* argmin_out,
                             int32_t* status_out, int mem, void* stream);
int igt_rollout_candidates_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                               const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc,
                               const double* U, double* X_all, double* U_all, double* cost_all, uint32_t* viol_all, int mem,
                               void* stream);

/* Rectangle (OBCA) collision model: the reference's collision_avoidance_type 'obca' (mpc.py:42-43, 105-106, 211-221) for the
 * shooting solver.  The reference certifies with dual variables that the ego rectangle and every obstacle rectangle are at
 * least d_box + 1e-6 apart; these entries judge that distance themselves.  Arguments are igt_solve_batch_ws_f64's /
 * igt_rollout_batch_ws_f64's, except:
 *   obs_pose [B,n_obs,3,N+1]   obstacle x, y, heading predictions (node 0 is not judged, as for obs_xy) in place of obs_xy;
 *   length, width, d_box       behind u_ws: the extents of every rectangle (ego and obstacles; the reference: 4.47, 2.0) and the
 *                              distance to keep (the reference: d_min = 0 in this mode);
 *   u_ws                       may be NULL.
 * The verdict, per obstacle o and node k = 1..N, with the ego's centre p = (x_k, y_k) and heading psi_k of the roll-out, the
 * obstacle's centre q and heading phi, half extents h = (length/2, width/2), rho = |h|:
 *   1. gate: |p - q|^2 >= (d_box + 1e-6 + 2 rho)^2 is clear, nothing else is evaluated;
 *   2. separating axes: t = R(psi)^T (q - p), theta = phi - psi, c = |cos theta|, s = |sin theta|; the depths
 *      h0 + h0 c + h1 s - |t0| and h1 + h0 s + h1 c - |t1|, the same two with the roles swapped (t' = R(phi)^T (p - q)); depth is
 *      the smallest of the four;
 *   3. signed gap: depth > 0, the rectangles overlap and gap = -depth (the penetration depth); else gap is the smallest, over
 *      the eight vertices of one rectangle taken in the other's frame, of |max(|v| - h, 0)| -- the distance of the rectangles;
 *   4. g = d_box + 1e-6 - gap is violated where g > feas_tol and reports IGT_VIOL_COLLISION.  (The gap is signed on purpose:
 *      with gap = 0 on overlap g would equal the default feas_tol exactly and an overlap would pass.)
 *   5. a non-finite obstacle coordinate or heading (|heading| beyond 1e6 counts) makes that node of that obstacle no constraint.
 * Every candidate family, both costs, refine_iters, the warm start, any N, n_rk4 and n_obs.  The calls are stateless: the handle
 * keeps nothing of them and the circle entries are untouched; with every obstacle beyond the gate the answers are those of the
 * circle entries without obstacles, bit for bit.  IGT_MEM_DEVICE: the call only enqueues; after one call at that B it neither
 * allocates nor synchronises (capturable), and a replayed graph reads what obs_pose holds at replay time.
 * IGT_E_INVALID, with a message that names the cause, for a null handle, B < 0, a length or width that is not finite and
 * positive, a d_box that is not finite or below 0, a handle with polish_iters > 0 or igt_set_value_polish > 0 (the polish
 * kernels judge their trial plans with the circle) and with the developer kernels of IGT_DEV_FLAGS 32 / 1024 / 2048; B = 0 is a
 * no-op.  Out of scope, each refused or simply absent: _f32 entries, the two polishes, per-scenario candidate sets, the
 * pooled search (a box solve runs every 64-candidate unit on a plain grid).  obs_pose comes from igt_forecast_scene_pose_f64 /
 * igt_forecast_batch_pose_f64 above.  (Added without a change of IGT_VERSION; callers probe the symbols.) */
int igt_solve_batch_box_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                            const uint32_t* flags, const double* obs_pose, const double* tv_sv, const double* enc,
                            const double* u_ws, double length, double width, double d_box, double* x_out, double* u_out,
                            double* cost_out, int32_t* argmin_out, int32_t* status_out, int mem, void* stream);
int igt_rollout_batch_box_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                              const uint32_t* flags, const double* obs_pose, const double* tv_sv, const double* enc,
                              const double* u_ws, double length, double width, double d_box, double* X_all, double* U_all,
                              double* cost_all, uint32_t* viol_all, int mem, void* stream);

/* The closed-loop step behind a solve: what the reference's driver does with every agent's answer before the next timestep
 * (evaluate.py:491-545), for n = E M agents in the row order of igt_forecast_scene_* / the solve's B.  Per agent i, with
 * ok = status[i] == 0:
 *   ok      x <- x_sol[i,:,1], u_prev <- u_sol[i,:,0] (widened to double)                              (evaluate.py:491-510)
 *   not ok  the brake fallback (evaluate.py:511-545): a_fb = a_brake where v = x[5] > 0, else 0; x <- one model step of
 *           (x, (a_fb, u_prev[1]), kparams) -- igt_frenet_step_f64's arithmetic and bits, with the handle's dt, n_rk4, l_r,
 *           l_f, in both entries --, u_prev <- (a_fb, u_prev[1]); where v < 0 instead x <- x with v = 0 and u_prev[0] <- 0
 *           (evaluate.py:523-526).  A NaN v takes neither comparison: a = 0 and the model step.
 *   has_plan[i] = ok; plan_x, plan_u = the solution as the agent shares it (utils.py:339-352) with NaN -> 0 and +-inf -> the
 *   largest finite value (torch.nan_to_num); the solver answers status 1 with NaN rows, so such an agent's plan is zeros
 *   u_ws = plan_u shifted by one step, the last column repeated (utils.py:354-363 augment_prev_sol): the next solve's warm start
 *   flags_out[i] = flags_in[i] | (ok ? IGT_FLAG_WARM : 0);   infeasible[i] += !ok
 *   the log (the reference driver's cl_traj [E,7M,T+1] and u_cl [E,2M,T] seen agent-major -- the same bytes): with t = *step in
 *   0 .. T_log - 1, u_log[i,:,t] = the new u_prev and x_log[i,:,t+1] = the new x; any other t writes nothing.
 * T is the precision of the solve that produced status / x_sol / u_sol; the state, kparams and the log are double in both.
 *   x [n,7] in/out   u_prev [n,2] in/out   kparams [n,3]   status [n]   x_sol [n,7,N+1]   u_sol [n,2,N]
 *   has_plan [n], plan_x [n,7,N+1], plan_u [n,2,N] out;  u_ws [n,2,N] out, may be NULL;  flags_in / flags_out [n], both or
 *   neither NULL;  infeasible [n] in/out, may be NULL;  x_log [n,7,T_log+1] / u_log [n,2,T_log], both or neither NULL;
 *   step: one int64 where the other buffers live, read only when logging.
 * No output may alias x_sol / u_sol; x and u_prev are updated in place.
 * IGT_MEM_DEVICE: one kernel enqueued on `stream`; no workspace, no allocation, no host synchronisation, nothing kept in the
 * handle (capturable; a replayed graph reads *step at replay time).  IGT_MEM_HOST: staged like every other entry; the counter
 * and the two log columns are then written by the host from the staged results, the logs are not copied.
 * IGT_E_INVALID for a null handle, n < 0, a bad mem, one buffer of a both-or-neither pair without the other, a log without
 * step, and -- n > 0 -- a null required buffer; n = 0 is a no-op.  (Added without a change of IGT_VERSION; callers probe the
 * symbols.) */
int igt_loop_advance_f64(igt_handle* h, int32_t n, double* x, double* u_prev, const double* kparams, const int32_t* status,
                         const double* x_sol, const double* u_sol, double a_brake, int32_t* has_plan, double* plan_x,
                         double* plan_u, double* u_ws, const uint32_t* flags_in, uint32_t* flags_out, int64_t* infeasible,
                         double* x_log, double* u_log, const int64_t* step, int32_t T_log, int mem, void* stream);
int igt_loop_advance_f32(igt_handle* h, int32_t n, double* x, double* u_prev, const double* kparams, const int32_t* status,
                         const float* x_sol, const float* u_sol, double a_brake, int32_t* has_plan, float* plan_x,
                         float* plan_u, float* u_ws, const uint32_t* flags_in, uint32_t* flags_out, int64_t* infeasible,
                         double* x_log, double* u_log, const int64_t* step, int32_t T_log, int mem, void* stream);

/* Workspace (owned by the handle, grown on the first solve of a batch size, never shrunk; growth synchronises the stream and is
 * refused under stream capture with IGT_E_STATE).  Per scenario, C = 256: 48 B of slice partials, 16 B of live-row masks and
 * incumbent keys (float64; float32: 8 B), 128 B of the acceleration rows' travel sums (float64), 768 B of horizon checkpoints of
 * the unit winners (float64, progress cost, N >= 8),
 * 288 B of queue order / counters; value-network cost: + 36 B per candidate (the list of feasible candidates).  Small float64
 * batches (no more 64-candidate units than the device has SIMDs: B <= 256 at C = 256) keep every candidate's trajectory for
 * the emit pass: 9 (N + 1) 64 doubles per unit = 97 KB per unit at N = 20, i.e. up to 99 MB per handle at B C / 64 = 1024.
 * Growth frees the old workspace, so it invalidates every stream graph captured on the handle before it (a replay would use the
 * freed addresses).  The size depends on the plan, not on B alone -- a float64 solve of B = 33 needs more than one of B = 4096 --:
 * before capturing, run once eagerly every kind of call the handle will serve while the graph is in use. */

/* Per-kernel timing with HIP events on the launch stream (used by bench.py for the
 * roofline line).  While enabled, every solve records events around its kernels;
 * igt_get_kernel_ms synchronises on them and returns the last call's durations. */
int igt_set_profiling(igt_handle* h, int enable);
int igt_get_kernel_ms(igt_handle* h, float* search_ms, float* emit_ms);

/* Algorithmic HBM bytes one solve moves: reads + writes. */
int igt_algorithmic_bytes_per_solve(const igt_handle* h, int elem_size, int64_t* read_bytes,
                                    int64_t* write_bytes);

#ifdef __cplusplus
}
#endif
#endif /* IGTMPC_H */
