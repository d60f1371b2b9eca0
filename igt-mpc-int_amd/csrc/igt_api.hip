// igt_api.hip -- the C ABI declared in include/igtmpc.h (handle management, argument
// validation, host staging, launches).  No exceptions cross the boundary.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "igt_launch.h"
#include "igt_stage.h"
#include "igtmpc.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(IGT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

}  // namespace

struct igt_handle {
    igt_params p;
    igt::KP kp;
    int device = 0;
    hipStream_t stream = nullptr;
    double* d_cinf = nullptr;
    double* d_table = nullptr;
    bool table_set = false;
    bool net_set = false;
    void* d_stage = nullptr;       // staging arena of the host-mode calls, laid out per call by a StagePlan (Staging below)
    size_t stage_bytes = 0;
    void* h_stage = nullptr;       // pinned mirror of the arena's first PACK_BYTES, allocated once (packed calls: one copy each way)
    void* d_work = nullptr;        // workspace: per-slice partial arg-min, value-net records
    size_t work_bytes = 0;
    double* d_routes = nullptr;    // [n_routes, 12] route geometry for the forecast kernel
    int n_routes = 0;
    double* d_heads = nullptr;     // [n_routes, 3] (h0, hN, abs) per route for the pose forecast (igt_set_route_headings); null: not set
    void* d_net = nullptr;         // value-net parameters (float block followed by double block)
    igt::DevNet<float> net_f;
    igt::DevNet<double> net_d;
    bool prof = false;
    hipEvent_t ev[3];
    bool ev_recorded = false;
    int n_cu = 256;                // compute units of the device (sizes the persistent search grid)
    int concurrency = 1;           // solves the caller keeps in flight on the device (igt_set_concurrency)
    int polish_grad = IGT_GRAD_FORWARD_DIFF;      // or IGT_GRAD_ADJOINT (igt_set_polish_gradient)
    int polish_step = IGT_POLISH_STEP_GRADIENT;   // or IGT_POLISH_STEP_NEWTON (igt_set_polish_step)
    int value_polish = 0;          // iterations of the polish under the value-network cost (igt_set_value_polish)
    void* comm = nullptr;          // RCCL communicator of igt_comm_init (null: none)
    int comm_world = 1, comm_rank = 0;
    int32_t comm_B_local = 0;      // shard size of the communicator's first all-gather (0 = none yet); later calls must match
    void* d_u0 = nullptr;          // [B_local,2] first-step controls staged for the all-gather
    size_t u0_bytes = 0;
    int dev_ckpt = -1;             // IGT_DEV_CKPT / IGT_DEV_TRAJ_MAX (threshold sweeps), read once at igt_create; -1: not set
    int dev_traj_max = -1;
    int dev_reserve_pool = -1, dev_reserve_units = -1;      // IGT_DEV_RESERVE / IGT_DEV_RESERVE_UNITS (developer library only); -1: not set
    int dev_poison = -1;           // IGT_DEV_POISON (0..255), read once at igt_create: every call that carves the workspace first fills
                                   // all of it with this byte (carve_work); -1: not set, nothing is enqueued
};

namespace {

// RCCL is bound at run time (dlopen), not at link time: a single-GPU user needs no RCCL at all, and a process that
// already carries one (torch ships its own librccl.so.1) must not get a second copy.
// Lifetime: the binding is opened by the first user -- igt_comm_unique_id for the length of the call, igt_comm_init for as
// long as its communicator lives -- and closed (dlclose) when the last communicator is destroyed (igt_comm_destroy /
// igt_destroy).  Nothing is left to static destructors: `g_rccl` is plain data, and at process exit no handle of the
// library refers to a DSO whose own teardown order it does not control ("exit-time abort").
struct IgtNcclId { char internal[IGT_COMM_ID_BYTES]; };
struct Rccl {
    void* lib;
    int users;
    int (*GetUniqueId)(IgtNcclId*);
    int (*CommInitRank)(void**, int, IgtNcclId, int);
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t);
    int (*CommDestroy)(void*);
    const char* (*GetErrorString)(int);
};
Rccl g_rccl = {nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
std::mutex g_rccl_mu;          // handles are per thread-group; two of them may reach igt_comm_* together

// one more user of the binding (opens it when there is none); null: RCCL cannot be loaded
Rccl* rccl_acquire() {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    Rccl& r = g_rccl;
    if (!r.lib) {
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names)
            if ((r.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;          // one the process already mapped
        for (int i = 0; !r.lib && i < 3; ++i) r.lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
        if (!r.lib) return nullptr;
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
        if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy) {
            dlclose(r.lib);
            r.lib = nullptr;
            return nullptr;
        }
    }
    ++r.users;
    return &r;
}
// the binding of a live communicator (its handle holds a use: never null while h->comm is set)
Rccl* rccl() { return g_rccl.lib ? &g_rccl : nullptr; }
void rccl_release() {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    Rccl& r = g_rccl;
    if (r.users > 0 && --r.users == 0 && r.lib) {
        dlclose(r.lib);          // drops this library's reference; a copy torch mapped stays mapped for torch
        r.lib = nullptr;
        r.GetUniqueId = nullptr; r.CommInitRank = nullptr; r.AllGather = nullptr; r.CommDestroy = nullptr; r.GetErrorString = nullptr;
    }
}
int rccl_fail(Rccl* r, const char* what, int rc) {
    return fail(IGT_E_HIP, std::string(what) + ": " + (r && r->GetErrorString ? r->GetErrorString(rc) : "RCCL error"));
}

int isqrt_exact(int c) {
    int g = (int)std::lround(std::sqrt((double)c));
    return g * g == c ? g : -1;
}

int validate(const igt_params& p, std::string& why) {
    if (p.N < 1 || p.N > IGT_MAX_N) { why = "N must be in [1, IGT_MAX_N]"; return -1; }
    if (p.n_rk4 < 1 || p.n_rk4 > 64) { why = "n_rk4 must be in [1, 64]"; return -1; }
    if (p.C < 64 || p.C % 64) { why = "C must be a positive multiple of 64"; return -1; }
    if (p.n_obs < 0 || p.n_obs > IGT_MAX_OBS) { why = "n_obs must be in [0, IGT_MAX_OBS]"; return -1; }
    if (!(p.dt > 0) || !(p.l_r > 0) || !(p.l_f > 0)) { why = "dt, l_r, l_f must be positive"; return -1; }
    {
        const double lim[] = {p.dt, p.l_r, p.l_f, p.v_min, p.v_max, p.a_min, p.a_max, p.df_max, p.jerk_limit,
                              p.steer_rate_limit, p.ey_lim, p.d_min, p.w_u, p.feas_tol};
        for (double x : lim)
            if (!std::isfinite(x)) { why = "dt, l_r, l_f, v_min, v_max, a_min, a_max, df_max, jerk_limit, steer_rate_limit, ey_lim, d_min, w_u and feas_tol must be finite"; return -1; }
    }
    if (!(p.jerk_limit > 0)) { why = "jerk_limit must be in (0, inf)"; return -1; }
    if (!(p.steer_rate_limit >= 0)) { why = "steer_rate_limit must be in [0, inf)"; return -1; }
    if (!(p.df_max < 1.5707963267948966)) { why = "df_max must be in [0, pi/2)"; return -1; }
    if (p.cand_mode == IGT_CAND_LATTICE) {
        const int g = isqrt_exact(p.C);
        if (g < 2 || 64 % g) { why = "lattice candidates need C = G*G with G in {2,4,8,16,32,64}; use IGT_CAND_TABLE"; return -1; }
    } else if (p.cand_mode == IGT_CAND_RAMP_HOLD || p.cand_mode == IGT_CAND_TRACK) {
        const int g = isqrt_exact(p.C);
        if (g < 4 || 64 % g) { why = "ramp-hold candidates need C = G*G with G in {4,8,16,32,64}"; return -1; }
    } else if (p.cand_mode != IGT_CAND_TABLE) {
        why = "unknown cand_mode"; return -1;
    }
    if (p.refine_iters < 0 || p.refine_iters > 4) { why = "refine_iters must be in [0, 4]"; return -1; }
    if (p.refine_iters > 0 && p.cand_mode != IGT_CAND_RAMP_HOLD && p.cand_mode != IGT_CAND_TRACK) { why = "refine_iters needs IGT_CAND_RAMP_HOLD or IGT_CAND_TRACK"; return -1; }
    if (p.polish_iters < 0 || p.polish_iters > 4) { why = "polish_iters must be in [0, 4]"; return -1; }
    if (p.polish_iters > 0 && p.cost_mode != IGT_COST_PROGRESS) { why = "polish_iters needs IGT_COST_PROGRESS (the value-network cost is not polished)"; return -1; }
    if (p.cand_mode == IGT_CAND_TRACK && (!(p.track_ke >= 0) || !(p.track_span >= 0) || !(p.track_beta_lim > 0) || !(p.track_beta_lim < 1.5) || !(p.track_env >= 0) || !(p.track_env < 1e6) || !(p.track_vcap >= 0) || !(p.track_vcap < 1e6))) { why = "track_ke, track_span, track_env, track_vcap must be >= 0 (and finite) and 0 < track_beta_lim < 1.5"; return -1; }
    if (p.cost_mode != IGT_COST_PROGRESS && p.cost_mode != IGT_COST_VALUE_NET) { why = "unknown cost_mode"; return -1; }
    if (!(p.v_min <= p.v_max) || !(p.a_min <= p.a_max) || !(p.df_max >= 0)) { why = "inconsistent limits"; return -1; }
    if (!(p.feas_tol >= 0)) { why = "feas_tol must be >= 0"; return -1; }
    return 0;
}

igt::KP make_kp(const igt_params& p, int F) {
    igt::KP k;
    k.N = p.N; k.n_rk4 = p.n_rk4; k.C = p.C; k.n_obs = p.n_obs;
    k.cand_mode = p.cand_mode; k.cost_mode = p.cost_mode; k.F = F;
    k.G = p.cand_mode == IGT_CAND_TABLE ? 1 : isqrt_exact(p.C);
    k.refine_it = 0;
    k.df_small = p.df_max < 0.78 ? 1 : 0;
    { const char* e = getenv("IGT_DEV_FLAGS"); k.dev = (e ? atoi(e) : 0) & igt::DEV_ENV_MASK; }      // (the launch-time bits are the launchers')
    k.dt = p.dt;
    k.h = p.dt / p.n_rk4;                      // frenet.py:93
    k.l_r = p.l_r;
    k.lr_ratio = p.l_r / (p.l_f + p.l_r);      // frenet.py:72
    k.v_min = p.v_min; k.v_max = p.v_max; k.a_min = p.a_min; k.a_max = p.a_max; k.df_max = p.df_max;
    k.rate_a = p.dt * p.jerk_limit;            // mpc.py:304
    k.rate_df = p.dt * p.steer_rate_limit;     // mpc.py:306
    k.ey_lim = p.ey_lim;
    k.dmin2 = p.d_min * p.d_min;               // mpc.py:226
    k.w_u = p.w_u;
    k.tol = p.feas_tol;
    k.trk_ke = p.track_ke; k.trk_span = p.track_span; k.trk_blim = p.track_beta_lim;
    // slope of the acceleration envelope (igt_device.h track_accel_target_uncapped); products and one quotient only, so the
    // oracle's track_env_slope() gives the same bits
    // The envelope is the stationary point of  w_u a_k^2 - (s_N - s_0)  (mpc.py:362, 372).  The gt_mpc cost has no
    // progress term (mpc.py:367-370: the value network stands there), so with IGT_COST_VALUE_NET it is not applied.
    k.trk_env = (p.track_env > 0 && p.w_u > 0 && p.cost_mode == IGT_COST_PROGRESS)
                    ? p.track_env * p.dt * p.dt / (2 * p.w_u) : (double)INFINITY;
    // speed cap of the acceleration targets (igt_device.h track_speed_cap): the speed it looks ahead to -- the box less a margin
    // far above a float32 roll-out's rounding (oracle: TRACK_VCAP_MARGIN) --, +inf when off
    k.trk_vmax = p.track_vcap > 0 ? p.v_max - 1e-4 : (double)INFINITY;
    k.inv_dt = 1.0 / p.dt;
    k.inv_rate_a = 1.0 / (p.dt * p.jerk_limit);
    // stage-offset polynomials: short form while h * (largest angular rate a candidate can reach) stays
    // small (igt_fast.h small_sincos2); v up to v_max + 2, |K| up to 0.25, sin(beta)/l_r <= 0.7/l_r
    const double vhi = std::fmax(std::fabs(p.v_min), std::fabs(p.v_max)) + 2.0;
    k.hi_order = (k.h * vhi * (0.7 / p.l_r + 0.25) > 0.12) ? 1 : 0;
    return k;
}

int ensure_stage(igt_handle* h, size_t bytes) {
    if (!h->h_stage) HIPCHK(hipHostMalloc(&h->h_stage, igt::PACK_BYTES, hipHostMallocDefault));
    if (bytes <= h->stage_bytes) return 0;
    if (h->d_stage) { HIPCHK(hipFree(h->d_stage)); h->d_stage = nullptr; h->stage_bytes = 0; }
    const size_t want = bytes + bytes / 4 + 4096;
    HIPCHK(hipMalloc(&h->d_stage, want));
    h->stage_bytes = want;
    return 0;
}

// true while `st` is recording a stream graph: nothing that synchronises or allocates may be issued then
bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

int ensure_work(igt_handle* h, size_t bytes, hipStream_t st) {
    if (bytes <= h->work_bytes) return 0;
    if (capturing(st))
        return fail(IGT_E_STATE, "workspace too small for stream capture: run one eager solve of this batch size (and "
                                 "cost / candidate mode) on this handle first");
    HIPCHK(hipStreamSynchronize(st));
    if (h->d_work) { HIPCHK(hipFree(h->d_work)); h->d_work = nullptr; h->work_bytes = 0; }
    const size_t want = bytes + bytes / 4 + 4096;
    HIPCHK(hipMalloc(&h->d_work, want));
    h->work_bytes = want;
    return 0;
}

template <typename T> const igt::DevNet<T>& net_of(const igt_handle* h);
template <> const igt::DevNet<float>& net_of<float>(const igt_handle* h) { return h->net_f; }
template <> const igt::DevNet<double>& net_of<double>(const igt_handle* h) { return h->net_d; }

// The buffers of one call that takes mem = IGT_MEM_HOST | IGT_MEM_DEVICE ("How an entry stages host
// buffers").  An entry declares each buffer once -- in(&device pointer, caller's array, elements[, copied]) or out(...) --,
// then upload(), its launches, download().  IGT_MEM_DEVICE: every pointer is handed back as it came and nothing is allocated,
// copied or synchronised, so such a call can be captured into a graph.  IGT_MEM_HOST: upload() lays the buffers out in
// h->d_stage (igt_stage.h StagePlan), points the device pointers there and copies the inputs; download() copies the outputs
// back and synchronises once.  With `pack` (the solve entries) a call of at most igt::PACK_BYTES crosses in one copy each way,
// through the pinned mirror.  A null array that would be copied is an absent optional buffer: its device pointer stays null.
class Staging {
public:
    Staging(igt_handle* h, int mem, void* stream, bool pack = false)
        : h_(h), mem_(mem), st_(stream ? (hipStream_t)stream : h->stream), pack_(pack) {}
    hipStream_t stream() const { return st_; }
    // The one `mem` check.  upload() makes it for every entry; terminal_value and cost_gradient_vn also call it themselves
    // ahead of their empty-batch return, because they refuse a bad `mem` even for n == 0 -- neither call is redundant.
    int check_mem() const {
        if (mem_ == IGT_MEM_DEVICE || mem_ == IGT_MEM_HOST) return IGT_OK;
        return fail(IGT_E_INVALID, "mem must be IGT_MEM_DEVICE or IGT_MEM_HOST");
    }
    template <typename U> void in(const U** dev, const U* host, size_t n, bool copy = true) {
        *dev = host;
        if (mem_ == IGT_MEM_HOST) add(dev, plan_.add(host, n * sizeof(U), sizeof(U), false, copy));
    }
    template <typename U> void out(U** dev, U* host, size_t n) {
        *dev = host;
        if (mem_ == IGT_MEM_HOST) add(dev, plan_.add(host, n * sizeof(U), sizeof(U), true));
    }
    // selects the device, refuses a bad `mem` (check_mem: here for the seven entries that answer an empty batch first), and
    // in host mode stages the inputs
    int upload() {
        HIPCHK(hipSetDevice(h_->device));
        if (int rc = check_mem()) return rc;
        if (mem_ == IGT_MEM_DEVICE) return IGT_OK;
        if (plan_.overflow) return fail(IGT_E_STATE, "more staged buffers than igt_stage.h STAGE_MAX_BUFFERS");
        plan_.layout();
        if (int rc = ensure_stage(h_, plan_.total)) return rc;
        char* base = static_cast<char*>(h_->d_stage);
        for (int i = 0; i < plan_.n; ++i) slot_[i].point(slot_[i].var, base + plan_.buf[i].off);
        packed_ = pack_ && plan_.packed();
        if (packed_) {
            plan_.gather(h_->h_stage);
            HIPCHK(hipMemcpyAsync(base, h_->h_stage, plan_.in_span, hipMemcpyHostToDevice, st_));
            return IGT_OK;
        }
        for (int i = 0; i < plan_.n; ++i) {
            const igt::StagePlan::Buf& b = plan_.buf[i];
            if (!b.out && b.copy) HIPCHK(hipMemcpyAsync(base + b.off, b.host, b.bytes, hipMemcpyHostToDevice, st_));
        }
        return IGT_OK;
    }
    int download() {
        if (mem_ != IGT_MEM_HOST) return IGT_OK;
        const char* base = static_cast<const char*>(h_->d_stage);
        if (packed_) {
            char* hs = static_cast<char*>(h_->h_stage);
            HIPCHK(hipMemcpyAsync(hs + plan_.out_begin, base + plan_.out_begin, plan_.total - plan_.out_begin,
                                  hipMemcpyDeviceToHost, st_));
            HIPCHK(hipStreamSynchronize(st_));
            plan_.scatter(hs);
            return IGT_OK;
        }
        for (int i = 0; i < plan_.n; ++i) {
            const igt::StagePlan::Buf& b = plan_.buf[i];
            if (b.out && b.copy) HIPCHK(hipMemcpyAsync(b.host, base + b.off, b.bytes, hipMemcpyDeviceToHost, st_));
        }
        HIPCHK(hipStreamSynchronize(st_));
        return IGT_OK;
    }

private:
    // remembers where buffer i's device pointer lives (P = const U* or U*), with the typed assignment that re-points it
    template <typename P> void add(P* dev, int i) {
        if (i >= 0) slot_[i] = Slot{dev, [](void* var, void* p) { *static_cast<P*>(var) = static_cast<P>(p); }};
    }
    struct Slot {
        void* var;
        void (*point)(void* var, void* p);
    };
    igt_handle* h_;
    int mem_;
    hipStream_t st_;
    bool pack_, packed_ = false;
    igt::StagePlan plan_;
    Slot slot_[igt::STAGE_MAX_BUFFERS];      // each buffer's device pointer, in the entry's frame
};

// Carves 256-byte aligned pieces out of the workspace.  A call's share is laid out by one carve function, run twice
// (carve_work): first on an arena with no base, which only adds up the bytes (the pointers it hands out are offsets and are
// never used), then -- once ensure_work has made the workspace that large -- on the workspace itself.
struct Arena {
    char* base;
    size_t off;
    template <typename U> U* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        U* p = reinterpret_cast<U*>(reinterpret_cast<uintptr_t>(base) + off);
        off += n * sizeof(U);
        return p;
    }
};
template <class Carve> int carve_work(igt_handle* h, hipStream_t st, const Carve& carve) {
    Arena sizing{nullptr, 0};
    carve(sizing);
    if (int rc = ensure_work(h, sizing.off, st)) return rc;
    // IGT_DEV_POISON: the whole workspace -- not this call's share alone -- holds one known byte before the entry's own memsets and
    // launches, so that a piece read before it is written shows as a wrong answer whatever the call before left there (DESIGN
    // section 6).  A memset node would change a captured graph: not under capture.
    if (h->dev_poison >= 0 && h->d_work && !capturing(st)) HIPCHK(hipMemsetAsync(h->d_work, h->dev_poison, h->work_bytes, st));
    Arena wa{(char*)h->d_work, 0};
    carve(wa);
    return IGT_OK;
}

// The argument checks solve and rollout-all share (each entry point checks its own outputs).  B == 0: IGT_OK with *empty set,
// nothing else is checked.  own_table: the call brings its candidates (check_candidates), the handle's table is not asked for.
int check_batch(const igt_handle* h, int32_t B, const void* x0, const void* u_prev, const void* kparams, const void* flags,
                const void* obs_xy, const void* tv_sv, const void* enc, const void* u_ws, bool* empty, bool own_table = false) {
    *empty = false;
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (B < 0) return fail(IGT_E_INVALID, "B < 0");
    if (B == 0) { *empty = true; return IGT_OK; }
    if (!x0 || !u_prev || !kparams || !flags) return fail(IGT_E_INVALID, "null buffer");
    const igt_params& p = h->p;
    if (p.n_obs > 0 && !obs_xy) return fail(IGT_E_INVALID, "obs_xy is null but n_obs > 0");
    if (p.cand_mode == IGT_CAND_TABLE && !h->table_set && !own_table) return fail(IGT_E_STATE, "candidate table not set");
    if (u_ws && p.cand_mode != IGT_CAND_RAMP_HOLD && p.cand_mode != IGT_CAND_TRACK)
        return fail(IGT_E_INVALID, "a warm start needs IGT_CAND_RAMP_HOLD or IGT_CAND_TRACK (the families whose targets are centred on it)");
    if (p.cost_mode == IGT_COST_VALUE_NET) {
        if (!h->net_set) return fail(IGT_E_STATE, "value net not set (igt_set_value_net)");
        if (!tv_sv || !enc) return fail(IGT_E_INVALID, "tv_sv / enc required for the value-net cost");
    }
    return IGT_OK;
}

// What igt_solve_candidates_f64 / igt_rollout_candidates_f64 refuse ahead of check_batch: U[B,C,2,N] stands in for the handle's
// table, so the handle must be of the table family (which fixes C and N); the oracle-order and literal developer kernels know
// one shared table only.
int check_candidates(const igt_handle* h, int32_t B, const void* U) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (B < 0) return fail(IGT_E_INVALID, "B < 0");
    if (!U && B > 0) return fail(IGT_E_INVALID, "U is null (per-scenario candidates U[B,C,2,N])");      // B == 0: an empty buffer
    if (h->p.cand_mode != IGT_CAND_TABLE)
        return fail(IGT_E_INVALID, "per-scenario candidates need a handle created with IGT_CAND_TABLE (it fixes C and N)");
    if (h->kp.dev & (igt::DEV_EXACT64 | igt::DEV_LITERAL))
        return fail(IGT_E_INVALID, "per-scenario candidates are not available with the developer kernels of IGT_DEV_FLAGS 1024 / 2048");
    return IGT_OK;
}

// What igt_solve_batch_box_f64 / igt_rollout_batch_box_f64 refuse ahead of check_batch, and the model the kernels take.  The
// polish kernels judge their trial plans with the circle, so a handle that polishes is refused; the developer kernels know the
// circle alone.
int check_box(const igt_handle* h, int32_t B, double length, double width, double d_box, igt::BoxModel* box) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (B < 0) return fail(IGT_E_INVALID, "B < 0");
    static_assert(IGT_MAX_OBS * IGT_MAX_N <= igt::BOX_TAB_MAX_ENTRIES, "fill_box_table's LDS holds every (obstacle, node)");
    if (const char* why = igt::box_model(length, width, d_box, box)) return fail(IGT_E_INVALID, why);
    if (h->p.polish_iters > 0)
        return fail(IGT_E_INVALID, "box collision model: polish_iters > 0 is not supported (the polish judges its trial plans with the circle)");
    if (h->value_polish > 0)
        return fail(IGT_E_INVALID, "box collision model: igt_set_value_polish > 0 is not supported (the polish judges its trial plans "
                                   "with the circle); igt_set_value_polish(h, 0) for a box solve");
    if (h->kp.dev & igt::DEV_KERNEL_FLAGS)
        return fail(IGT_E_INVALID, "box collision model: not available with the developer kernels of IGT_DEV_FLAGS 32 / 1024 / 2048");
    return IGT_OK;
}

// box (igt_solve_batch_box_f64, T = double): obs_xy is the poses [B,n_obs,3,N+1] and the search is plan_box64's
template <typename T>
int solve_impl(igt_handle* h, int32_t B, const T* x0, const T* u_prev, const T* kparams, const uint32_t* flags,
               const T* obs_xy, const T* tv_sv, const T* enc, const T* u_ws, T* x_out, T* u_out, T* cost_out,
               int32_t* argmin_out, int32_t* status_out, int mem, void* stream, const double* U_own = nullptr,
               const igt::BoxModel* box = nullptr) {
    // U_own (igt_solve_candidates_f64, T = double): the candidates U[B,C,2,N], staged like the other inputs, in place of the
    // handle's table -- the search and emit of plan_candidates64, everything behind the emit as for any table handle
    bool empty;
    if (int rc = check_batch(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, u_ws, &empty, U_own != nullptr)) return rc;
    if (empty) return IGT_OK;
    if (!x_out || !u_out || !cost_out || !argmin_out || !status_out) return fail(IGT_E_INVALID, "null buffer");
    const igt_params& p = h->p;
    if (p.polish_iters > 0 && sizeof(T) == 4)
        return fail(IGT_E_INVALID, "polish_iters > 0 needs the _f64 entry points (a forward difference of 1e-4 on a float cost is noise)");
    if (p.polish_iters > 0 && (h->kp.dev & (igt::DEV_EXACT64 | igt::DEV_LITERAL)))
        return fail(IGT_E_INVALID, "polish_iters > 0 is not available with the developer kernels of IGT_DEV_FLAGS 1024 / 2048");
    // polish under the value-network cost (igt_set_value_polish): refused before anything is staged or enqueued
    const int vp_iters = h->value_polish;
    if (vp_iters > 0) {
        if (sizeof(T) == 4) return fail(IGT_E_INVALID, "igt_set_value_polish > 0 needs the _f64 entry points");
        if (h->kp.dev & (igt::DEV_EXACT64 | igt::DEV_LITERAL))
            return fail(IGT_E_INVALID, "igt_set_value_polish > 0 is not available with the developer kernels of IGT_DEV_FLAGS 1024 / 2048");
        if (B > igt::VALUE_POLISH_MAX_B) return fail(IGT_E_INVALID, "igt_set_value_polish > 0: B exceeds the 64 B trial records an int counts");
        if (capturing(stream ? (hipStream_t)stream : h->stream))
            return fail(IGT_E_STATE, "igt_set_value_polish > 0 cannot be recorded under stream capture: a solve replayed from a stream "
                                     "graph with this polish faulted and the cause is not known; igt_set_value_polish(h, 0) for a "
                                     "captured solve");
    }
    const bool value = p.cost_mode == IGT_COST_VALUE_NET;
    const size_t n_x = (size_t)B * 7, n_u = (size_t)B * 2, n_k = (size_t)B * 3;
    const size_t n_obs = (size_t)B * p.n_obs * (box ? 3 : 2) * (p.N + 1);
    const size_t n_xo = (size_t)B * 7 * (p.N + 1), n_uo = (size_t)B * 2 * p.N;

    igt::SolveArgs<T> A{};
    if (box) A.box = *box;
    A.table = h->table_set ? h->d_table : nullptr;
    A.cinf = h->kp.F > 0 ? h->d_cinf : nullptr;
    Staging stg(h, mem, stream, /*pack=*/true);
    stg.in(&A.x0, x0, n_x); stg.in(&A.u_prev, u_prev, n_u); stg.in(&A.kparams, kparams, n_k);
    stg.in(&A.flags, flags, (size_t)B); stg.in(&A.obs, obs_xy, n_obs);
    stg.in(&A.tv_sv, tv_sv, n_u, value); stg.in(&A.enc, enc, n_u, value);
    stg.in(&A.u_ws, u_ws, n_uo);
    if (U_own) {
        A.table_stride = igt::cand_table_doubles(p.C, p.N);
        stg.in(&A.table, U_own, (size_t)B * A.table_stride);
    }
    stg.out(&A.x_out, x_out, n_xo); stg.out(&A.u_out, u_out, n_uo); stg.out(&A.cost_out, cost_out, (size_t)B);
    stg.out(&A.argmin_out, argmin_out, (size_t)B); stg.out(&A.status_out, status_out, (size_t)B);
    if (int rc = stg.upload()) return rc;
    hipStream_t st = stg.stream();

    // Which kernels search and emit run, and with them the partials, checkpoints, trajectories and queue order to carve and the
    // memsets of a pass: decided once, in igt_launch.h (plan_search32, plan_search64, plan_candidates64).  One plan for the
    // solve: a refinement pass changes nothing it reads.
    A.n_cu = h->n_cu;
    const int waves_per_simd = h->concurrency >= 3 ? 1 : 2;      // two solves in flight do not overlap on this runtime (igtmpc.h)
    if constexpr (sizeof(T) == 4)
        A.plan = igt::plan_search32(h->kp, B, value, igt::Search32Env{h->n_cu, waves_per_simd, h->dev_ckpt});
    else
        A.plan = U_own ? igt::plan_candidates64(h->kp, B, value)
                 : box ? igt::plan_box64(h->kp, B, value)
                       : igt::plan_search64(h->kp, B, value, igt::Search64Env{h->n_cu, waves_per_simd, h->dev_reserve_pool,
                                                                               h->dev_reserve_units, h->dev_traj_max});
    const auto& plan = A.plan;
    const size_t Wk = (size_t)plan.W, W = (size_t)plan.partials;      // units and partials per scenario
    const bool exact64 = sizeof(T) == 8 && (h->kp.dev & igt::DEV_EXACT64);      // developer switch: oracle-order double kernels
    const bool trace = (h->kp.dev & igt::DEV_TRACE) != 0;      // developer trace: 32 B per unit behind the counters
    const size_t n_rec = value ? (size_t)B * p.C : 0;
    double* d_cpar = nullptr;
    double* vp_work = nullptr;      // igt_value_polish_layout.h: the scratch of igt_set_value_polish's iterations
    // workspace (grows on first use, never shrinks): per-unit partial arg-min [+ value-net records]
    const auto carve = [&](Arena& wa) {
        A.part_J = wa.take<double>(igt::PartJTail<T>(nullptr, B, (int)W, h->kp.G).doubles(plan.ck_records != 0));
        const igt::PartJTail<T> tail(A.part_J, B, (int)W, h->kp.G);
        A.incumbents = tail.incumbents();
        if constexpr (sizeof(T) == 8) {
            A.row_mask = tail.masks();
            A.row_rems = tail.row_rems();
            A.ck_records = plan.ck_records ? tail.ck_records() : nullptr;
        }
        A.part_c = wa.take<int32_t>((size_t)B * W);
        d_cpar = wa.take<double>((size_t)B * 4);
        A.work_counter = wa.take<unsigned>(igt::WORK_COUNTER_WORDS + (trace ? (size_t)((B + 7) / 8) * 8 * Wk * 8 : 0));
        A.ckpt = plan.ckpt_doubles ? wa.take<double>(plan.ckpt_doubles) : nullptr;
        A.queue_order = plan.queue_order_words ? wa.take<unsigned>(plan.queue_order_words) : nullptr;
        A.traj = plan.traj_doubles ? wa.take<double>(plan.traj_doubles) : nullptr;
        if (value) {
            A.rec_J = wa.take<double>(n_rec);
            A.rec_sN = wa.take<T>(n_rec);
            A.rec_vN = wa.take<T>(n_rec);
            A.rec_viol = wa.take<uint32_t>(n_rec);
            A.p_vec = wa.take<T>((size_t)B * igt::VN_H);
            A.rec_b = wa.take<int32_t>(n_rec);
            A.rec_count = wa.take<unsigned>(64);
            A.best_key = wa.take<unsigned long long>((size_t)B);
            A.unit_seg = wa.take<int2>((size_t)B * Wk);
            if (sizeof(T) == 8) {
                A.prune_thr = wa.take<double>((size_t)B);
                A.live_idx = wa.take<unsigned>(n_rec);
            }
        }
        if (vp_iters > 0) vp_work = wa.take<double>(igt::ValuePolishLayout::doubles(B, p.N));      // behind everything else
    };
    if (int rc = carve_work(h, st, carve)) return rc;
    if (h->prof) HIPCHK(hipEventRecord(h->ev[0], st));
    igt::KP kp = h->kp;
    for (int it = 0; it <= p.refine_iters; ++it) {
        kp.refine_it = it;
        A.cpar = it == 0 ? nullptr : d_cpar;
        // the unit counters where no queue builder zeroes them; the compact list of feasible candidates (both precisions) and
        // the float path's per-scenario keys
        if (plan.memset_counters) HIPCHK(hipMemsetAsync(A.work_counter, 0, 8 * 256, st));
        if (plan.reset_rec_count) HIPCHK(hipMemsetAsync(A.rec_count, 0, 256, st));
        if (plan.reset_best_key) HIPCHK(hipMemsetAsync(A.best_key, 0xff, (size_t)B * 8, st));
        if (value) {
            HIPCHK(igt::launch_search_records<T>(kp, B, A, st));
            HIPCHK(igt::launch_value<T>(kp, B, net_of<T>(h), A, nullptr, nullptr, st));
            if (exact64) HIPCHK(igt::launch_reduce<T>(B, (int)W, A, st));
        } else {
            HIPCHK(igt::launch_search<T>(kp, B, A, st));
        }
        if (it < p.refine_iters) {   // winner of this pass -> centre / span of the next one
            igt::SolveArgs<T> R = A;
            int Wr = (int)W;
            if (exact64 && !value) {   // oracle-order double kernels, progress cost: the search already reduced to one winner
                R.part_J = reinterpret_cast<double*>(A.cost_out);
                R.part_c = A.argmin_out;
                Wr = 1;
            }
            HIPCHK(igt::launch_refine<T>(kp, B, Wr, R, d_cpar, it == 0 ? 1 : 0, st));
        }
    }
    if (h->prof) HIPCHK(hipEventRecord(h->ev[1], st));
    HIPCHK(igt::launch_emit<T>(kp, B, (int)W, A, st));
    if constexpr (sizeof(T) == 8) {      // the winners, polished in place in the outputs (igt_kernels_f64.hip polish_f64_kernel)
        if (p.polish_iters > 0) HIPCHK(igt::launch_polish(kp, B, p.polish_iters, h->polish_grad == IGT_GRAD_ADJOINT,
                                                       h->polish_step == IGT_POLISH_STEP_NEWTON, A, st));
        // igt_set_value_polish: six launches an iteration, each sized by B (igt_kernels_f64.hip value_trials_f64_kernel) -- the
        // gradient at the plan as igt_cost_gradient_vn_f64 takes it, the 64 trials per scenario, their values, the acceptance
        if (vp_iters > 0) {
            const igt::ValuePolishLayout VL(B, p.N);
            double* grad = vp_work + VL.grad();
            double* vn = vp_work + VL.vn();
            const igt::VnScratch S(vn, B);
            for (int it = 0; it < vp_iters; ++it) {
                HIPCHK(igt::launch_cost_gradient_vn(kp, B, true, A.x0, A.kparams, A.u_out, vp_work + VL.grad_cost(), grad, vn, st));
                HIPCHK(igt::launch_terminal_value(h->net_d, h->n_cu, B, S.sv(), A.tv_sv, A.enc, S.V(), S.dV(), st));
                HIPCHK(igt::launch_cost_gradient_vn(kp, B, false, A.x0, A.kparams, A.u_out, vp_work + VL.grad_cost(), grad, vn, st));
                HIPCHK(igt::launch_value_trials(kp, B, it == 0, A, vp_work, st));
                HIPCHK(igt::launch_terminal_value(h->net_d, h->n_cu, B * igt::VALUE_POLISH_TRIALS, vp_work + VL.sv(),
                                                  vp_work + VL.tv_sv(), vp_work + VL.enc(), vp_work + VL.V(), nullptr, st));
                HIPCHK(igt::launch_value_accept(kp, B, A, vp_work, st));
            }
        }
    }
    if (h->prof) { HIPCHK(hipEventRecord(h->ev[2], st)); h->ev_recorded = true; }

    if (h->kp.dev & igt::DEV_TRACE) {      // developer trace -> $IGT_DEV_TRACE (binary u64[units][4])
        if (const char* path = std::getenv("IGT_DEV_TRACE")) {
            HIPCHK(hipStreamSynchronize(st));
            const size_t n = (size_t)((B + 7) / 8) * 8 * Wk * 4;
            std::vector<unsigned long long> tr(n);
            HIPCHK(hipMemcpy(tr.data(), igt::unit_trace(A.work_counter), n * 8, hipMemcpyDeviceToHost));
            if (FILE* f = std::fopen(path, "wb")) { std::fwrite(tr.data(), 8, n, f); std::fclose(f); }
        }
    }
    return stg.download();
}

template <typename T>
int rollout_impl(igt_handle* h, int32_t B, const T* x0, const T* u_prev, const T* kparams, const uint32_t* flags,
                 const T* obs_xy, const T* tv_sv, const T* enc, const T* u_ws, T* X_all, T* U_all, T* cost_all,
                 uint32_t* viol_all, int mem, void* stream, const double* U_own = nullptr, const igt::BoxModel* box = nullptr) {
    bool empty;      // U_own (igt_rollout_candidates_f64), box (igt_rollout_batch_box_f64): as in solve_impl
    if (int rc = check_batch(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, u_ws, &empty, U_own != nullptr)) return rc;
    if (empty) return IGT_OK;
    if (!cost_all || !viol_all) return fail(IGT_E_INVALID, "null buffer");
    const igt_params& p = h->p;
    const bool value = p.cost_mode == IGT_COST_VALUE_NET;
    const size_t n_x = (size_t)B * 7, n_u = (size_t)B * 2, n_k = (size_t)B * 3;
    const size_t n_obs = (size_t)B * p.n_obs * (box ? 3 : 2) * (p.N + 1);
    const size_t n_X = (size_t)B * p.C * 7 * (p.N + 1), n_U = (size_t)B * p.C * 2 * p.N, n_c = (size_t)B * p.C;
    igt::SolveArgs<T> A{};
    if (box) A.box = *box;
    A.table = h->table_set ? h->d_table : nullptr;
    A.cinf = h->kp.F > 0 ? h->d_cinf : nullptr;
    T *dX, *dU, *dc;
    uint32_t* dv;
    Staging stg(h, mem, stream);
    stg.in(&A.x0, x0, n_x); stg.in(&A.u_prev, u_prev, n_u); stg.in(&A.kparams, kparams, n_k);
    stg.in(&A.flags, flags, (size_t)B); stg.in(&A.obs, obs_xy, n_obs);
    stg.in(&A.tv_sv, tv_sv, n_u, value); stg.in(&A.enc, enc, n_u, value);
    stg.in(&A.u_ws, u_ws, (size_t)B * 2 * p.N);
    if (U_own) {
        A.table_stride = igt::cand_table_doubles(p.C, p.N);
        stg.in(&A.table, U_own, (size_t)B * A.table_stride);
    }
    stg.out(&dX, X_all, n_X); stg.out(&dU, U_all, n_U);      // optional: null = not wanted
    stg.out(&dc, cost_all, n_c); stg.out(&dv, viol_all, n_c);
    if (int rc = stg.upload()) return rc;
    hipStream_t st = stg.stream();
    if (value) {   // records -> value_kernel fills cost_all / viol_all with the terminal term included
        const auto carve = [&](Arena& wa) {
            A.rec_J = wa.take<double>(n_c);
            A.rec_sN = wa.take<T>(n_c);
            A.rec_vN = wa.take<T>(n_c);
            A.rec_viol = wa.take<uint32_t>(n_c);
            A.p_vec = wa.take<T>((size_t)B * igt::VN_H);
        };
        if (int rc = carve_work(h, st, carve)) return rc;
    }
    HIPCHK(igt::launch_rollout_all<T>(h->kp, B, A, dX, dU, dc, dv, st));
    if (value) HIPCHK(igt::launch_value<T>(h->kp, B, net_of<T>(h), A, dc, dv, st));
    return stg.download();
}

template <typename T>
int frenet_step_impl(igt_handle* h, int32_t n, const T* x, const T* u, const T* kparams, T* x_next, int mem,
                     void* stream) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (n < 0) return fail(IGT_E_INVALID, "negative size");
    if (n == 0) return IGT_OK;
    if (!x || !u || !kparams || !x_next) return fail(IGT_E_INVALID, "null buffer");
    const size_t n_x = (size_t)n * 7, n_u = (size_t)n * 2, n_k = (size_t)n * 3;
    const T *dx, *du, *dk;
    T* dout;
    Staging stg(h, mem, stream);
    stg.in(&dx, x, n_x); stg.in(&du, u, n_u); stg.in(&dk, kparams, n_k);
    stg.out(&dout, x_next, n_x);
    if (int rc = stg.upload()) return rc;
    HIPCHK(igt::launch_frenet_step<T>(h->kp, n, dx, du, dk, dout, stg.stream()));
    return stg.download();
}

// The closed-loop step behind a solve: one launch of loop_advance_kernel, nothing carved and nothing kept.  Host mode stages x and
// u_prev twice, as input and as output (the kernel reads the one and writes the other); the counter and the two log columns need
// only what the call brings back, so the host writes them itself and the logs never cross the bus.
template <typename T>
int loop_advance_impl(igt_handle* h, int32_t n, double* x, double* u_prev, const double* kparams, const int32_t* status,
                      const T* x_sol, const T* u_sol, double a_brake, int32_t* has_plan, T* plan_x, T* plan_u, T* u_ws,
                      const uint32_t* flags_in, uint32_t* flags_out, int64_t* infeasible, double* x_log, double* u_log,
                      const int64_t* step, int32_t T_log, int mem, void* stream) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (n < 0) return fail(IGT_E_INVALID, "n < 0");
    Staging stg(h, mem, stream);
    if (int rc = stg.check_mem()) return rc;      // (refused for an empty batch as well)
    if (!flags_in != !flags_out) return fail(IGT_E_INVALID, "flags_in and flags_out go together");
    if (!x_log != !u_log) return fail(IGT_E_INVALID, "x_log and u_log go together");
    if (x_log && !step) return fail(IGT_E_INVALID, "logging needs step");
    if (n == 0) return IGT_OK;
    if (!x || !u_prev || !kparams || !status || !x_sol || !u_sol) return fail(IGT_E_INVALID, "null buffer");
    if (!has_plan || !plan_x || !plan_u) return fail(IGT_E_INVALID, "null output buffer (has_plan, plan_x, plan_u)");
    const int N = h->p.N;
    const size_t n_x = (size_t)n * 7, n_u = (size_t)n * 2, n_k = (size_t)n * 3;
    const size_t n_sx = n_x * (N + 1), n_su = n_u * N;
    const bool host = mem == IGT_MEM_HOST;
    igt::LoopArgs<T> A{};
    A.a_brake = a_brake;
    stg.in(&A.x_in, (const double*)x, n_x); stg.in(&A.u_in, (const double*)u_prev, n_u); stg.in(&A.kparams, kparams, n_k);
    stg.in(&A.status, status, (size_t)n); stg.in(&A.x_sol, x_sol, n_sx); stg.in(&A.u_sol, u_sol, n_su);
    stg.in(&A.flags_in, flags_in, (size_t)n);
    stg.out(&A.x_out, x, n_x); stg.out(&A.u_out, u_prev, n_u); stg.out(&A.has_plan, has_plan, (size_t)n);
    stg.out(&A.plan_x, plan_x, n_sx); stg.out(&A.plan_u, plan_u, n_su); stg.out(&A.u_ws, u_ws, n_su);
    stg.out(&A.flags_out, flags_out, (size_t)n);
    if (!host) {
        A.infeasible = infeasible;
        A.x_log = x_log; A.u_log = u_log; A.step = step; A.T_log = T_log;
    }
    if (int rc = stg.upload()) return rc;
    HIPCHK(igt::launch_loop_advance<T>(h->kp, n, A, stg.stream()));
    if (int rc = stg.download()) return rc;
    if (host) {
        if (infeasible)
            for (int32_t i = 0; i < n; ++i) infeasible[i] += status[i] != 0;
        if (x_log && *step >= 0 && *step < (int64_t)T_log) {
            const size_t t = (size_t)*step, Tl = (size_t)T_log;
            for (size_t r = 0; r < n_x; ++r) x_log[r * (Tl + 1) + t + 1] = x[r];
            for (size_t r = 0; r < n_u; ++r) u_log[r * Tl + t] = u_prev[r];
        }
    }
    return IGT_OK;
}

int cost_gradient_impl(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags, const double* U,
                       double* cost_out, double* grad_out, int mem, void* stream) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (h->p.cost_mode != IGT_COST_PROGRESS)
        return fail(IGT_E_INVALID, "the cost gradient is that of IGT_COST_PROGRESS (the value-network cost is not differentiated)");
    if (B < 0) return fail(IGT_E_INVALID, "B < 0");
    if (B == 0) return IGT_OK;
    if (!cost_out || !grad_out) return fail(IGT_E_INVALID, "null output buffer (cost_out, grad_out)");
    if (!x0 || !kparams || !flags || !U) return fail(IGT_E_INVALID, "null buffer");
    const size_t n_x = (size_t)B * 7, n_k = (size_t)B * 3, n_u = (size_t)B * 2 * h->p.N;
    const double *dx, *dk, *du;
    double *dc, *dg;
    Staging stg(h, mem, stream);
    stg.in(&dx, x0, n_x); stg.in(&dk, kparams, n_k); stg.in(&du, U, n_u);
    stg.out(&dc, cost_out, (size_t)B); stg.out(&dg, grad_out, n_u);
    if (int rc = stg.upload()) return rc;
    // the flags only act on psi_0, which the progress cost never reads (igt_kernels_f64.hip cost_gradient_f64_kernel)
    HIPCHK(igt::launch_cost_gradient(h->kp, B, dx, dk, du, dc, dg, stg.stream()));
    return stg.download();
}

// what the two value-network gradient entries refuse before they look at their buffers
int check_value_handle(const igt_handle* h, const char* what) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (h->p.cost_mode != IGT_COST_VALUE_NET)
        return fail(IGT_E_INVALID, std::string(what) + " needs a handle created with IGT_COST_VALUE_NET");
    return IGT_OK;
}

int terminal_value_impl(igt_handle* h, int32_t n, const double* sv, const double* tv_sv, const double* enc, double* V_out,
                        double* dV_out, int mem, void* stream) {
    if (int rc = check_value_handle(h, "igt_terminal_value_f64")) return rc;
    if (n < 0) return fail(IGT_E_INVALID, "n < 0");
    Staging stg(h, mem, stream);
    if (int rc = stg.check_mem()) return rc;      // (refused for an empty batch as well)
    if (n == 0) return IGT_OK;
    if (!V_out) return fail(IGT_E_INVALID, "null output buffer (V_out)");
    if (!sv || !tv_sv || !enc) return fail(IGT_E_INVALID, "null buffer");
    if (!h->net_set) return fail(IGT_E_STATE, "value net not set (igt_set_value_net)");
    const size_t n2 = (size_t)n * 2;
    const double *ds, *dt, *de;
    double *dV, *dG;
    stg.in(&ds, sv, n2); stg.in(&dt, tv_sv, n2); stg.in(&de, enc, n2);
    stg.out(&dV, V_out, (size_t)n); stg.out(&dG, dV_out, n2);      // dV_out is optional
    if (int rc = stg.upload()) return rc;
    HIPCHK(igt::launch_terminal_value(h->net_d, h->n_cu, n, ds, dt, de, dV, dG, stg.stream()));
    return stg.download();
}

// Three launches: the forward sweep leaves (s_N, v_N) in the workspace, the network answers V_out and its
// partials there, and the sweep kernel runs again with that terminal seed.  The scratch is VnScratch (igt_launch.h), carved
// from the handle's workspace like a solve's: it grows on first use and cannot grow under stream capture.
int cost_gradient_vn_impl(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags,
                          const double* tv_sv, const double* enc, const double* U, double* cost_out, double* grad_out, int mem,
                          void* stream) {
    if (int rc = check_value_handle(h, "igt_cost_gradient_vn_f64")) return rc;
    if (B < 0) return fail(IGT_E_INVALID, "B < 0");
    Staging stg(h, mem, stream);
    if (int rc = stg.check_mem()) return rc;      // (refused for an empty batch as well)
    if (B == 0) return IGT_OK;
    if (!cost_out || !grad_out) return fail(IGT_E_INVALID, "null output buffer (cost_out, grad_out)");
    if (!x0 || !kparams || !flags || !U) return fail(IGT_E_INVALID, "null buffer");
    if (!tv_sv || !enc) return fail(IGT_E_INVALID, "tv_sv / enc required for the value-net cost");
    if (!h->net_set) return fail(IGT_E_STATE, "value net not set (igt_set_value_net)");
    const size_t n_x = (size_t)B * 7, n_k = (size_t)B * 3, n_2 = (size_t)B * 2, n_u = (size_t)B * 2 * h->p.N;
    const double *dx, *dk, *du, *dt, *de;
    double *dc, *dg;
    stg.in(&dx, x0, n_x); stg.in(&dk, kparams, n_k); stg.in(&du, U, n_u);
    stg.in(&dt, tv_sv, n_2); stg.in(&de, enc, n_2);
    stg.out(&dc, cost_out, (size_t)B); stg.out(&dg, grad_out, n_u);
    if (int rc = stg.upload()) return rc;
    hipStream_t st = stg.stream();
    double* vn = nullptr;
    const auto carve = [&](Arena& wa) { vn = wa.take<double>(igt::VnScratch::doubles(B)); };
    if (int rc = carve_work(h, st, carve)) return rc;
    const igt::VnScratch S(vn, B);
    // the flags only act on psi_0, which neither the stage terms nor the network's features read
    HIPCHK(igt::launch_cost_gradient_vn(h->kp, B, true, dx, dk, du, dc, dg, vn, st));
    HIPCHK(igt::launch_terminal_value(h->net_d, h->n_cu, B, S.sv(), dt, de, S.V(), S.dV(), st));
    HIPCHK(igt::launch_cost_gradient_vn(h->kp, B, false, dx, dk, du, dc, dg, vn, st));
    return stg.download();
}

// POSE (igt_forecast_batch_pose_f64, T = double): obs_xy is obs_pose[B,n_obs,3,N+1] and opp_heading[B,n_obs] is read
template <typename T, bool POSE = false>
int forecast_impl(igt_handle* h, int32_t B, const T* ego_xyh, const T* opp, const T* opp_a, const int32_t* opp_route,
                  const T* opp_heading, const T* plan_x, const T* plan_u, const int32_t* has_plan, T* obs_xy, T* tv_sv, int mem,
                  void* stream) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (B < 0) return fail(IGT_E_INVALID, "B < 0");
    if (B == 0) return IGT_OK;
    if (!h->d_routes) return fail(IGT_E_STATE, "route table not set (igt_set_routes)");
    if (POSE && !h->d_heads) return fail(IGT_E_INVALID, "route headings not set (igt_set_route_headings)");
    if (h->p.n_obs < 1) return fail(IGT_E_INVALID, "the forecast entry needs at least one other vehicle (n_obs >= 1)");
    if (!ego_xyh || !opp || !opp_a || !opp_route || !obs_xy || !tv_sv || (POSE && !opp_heading)) return fail(IGT_E_INVALID, "null buffer");
    const bool plans = plan_x && plan_u && has_plan;
    if (!plans && (plan_x || plan_u || has_plan)) return fail(IGT_E_INVALID, "plan_x, plan_u, has_plan go together");
    const int N = h->p.N;
    const size_t M1 = (size_t)h->p.n_obs;            // other vehicles per scene: every per-opponent array is [B, n_obs, ...]
    const size_t n_e = (size_t)B * 3, n_o = (size_t)B * M1 * 4, n_pairs = (size_t)B * M1;
    const size_t n_px = plans ? n_pairs * 7 * (N + 1) : 0, n_pu = plans ? n_pairs * 2 * N : 0;      // without plans: reserved only
    const size_t n_out = n_pairs * (POSE ? 3 : 2) * (N + 1), n_tv = n_pairs * 2;
    const T *de, *dop, *da, *dpx, *dpu, *dh = nullptr;
    const int32_t *dr, *dhp;
    T *dout, *dtv;
    Staging stg(h, mem, stream);
    stg.in(&de, ego_xyh, n_e); stg.in(&dop, opp, n_o); stg.in(&da, opp_a, n_pairs); stg.in(&dr, opp_route, n_pairs);
    if constexpr (POSE) stg.in(&dh, opp_heading, n_pairs);
    stg.in(&dhp, has_plan, n_pairs, plans); stg.in(&dpx, plan_x, n_px); stg.in(&dpu, plan_u, n_pu);
    stg.out(&dout, obs_xy, n_out); stg.out(&dtv, tv_sv, n_tv);
    if (int rc = stg.upload()) return rc;
    if constexpr (POSE)
        HIPCHK(igt::launch_forecast_pose(h->kp, B, h->d_routes, h->n_routes, h->d_heads, de, dop, da, dr, dh, plans ? dpx : nullptr,
                                         plans ? dpu : nullptr, plans ? dhp : nullptr, dout, dtv, stg.stream()));
    else
        HIPCHK(igt::launch_forecast<T>(h->kp, B, h->d_routes, h->n_routes, de, dop, da, dr, plans ? dpx : nullptr,
                                       plans ? dpu : nullptr, plans ? dhp : nullptr, dout, dtv, stg.stream()));
    return stg.download();
}

// POSE (igt_forecast_scene_pose_f64, T = double): obs_xy is obs_pose[E M,n_obs,3,N+1]
template <typename T, bool POSE = false>
int forecast_scene_impl(igt_handle* h, int32_t E, const T* x, const T* a_prev, const int32_t* route, const T* plan_x,
                        const T* plan_u, const int32_t* has_plan, T* obs_xy, T* tv_sv, int mem, void* stream) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (E < 0) return fail(IGT_E_INVALID, "E < 0");
    if (!h->d_routes) return fail(IGT_E_INVALID, "route table not set (igt_set_routes)");
    if (POSE && !h->d_heads) return fail(IGT_E_INVALID, "route headings not set (igt_set_route_headings)");
    if (h->p.n_obs < 1) return fail(IGT_E_INVALID, "the forecast entry needs at least one other vehicle (n_obs >= 1)");
    if (E == 0) return IGT_OK;
    if (!x || !a_prev || !route || !obs_xy || !tv_sv) return fail(IGT_E_INVALID, "null buffer");
    const bool plans = plan_x && plan_u && has_plan;
    if (!plans && (plan_x || plan_u || has_plan)) return fail(IGT_E_INVALID, "plan_x, plan_u, has_plan go together");
    const int N = h->p.N;
    const size_t M = (size_t)h->p.n_obs + 1;         // agents per scene; problem e M + i = agent i of scene e as ego
    if ((size_t)E > (size_t)0x7fffffff / (M * (M - 1))) return fail(IGT_E_INVALID, "E (n_obs + 1) n_obs exceeds int32");
    const size_t n_ag = (size_t)E * M, n_x = n_ag * 7;
    const size_t n_px = plans ? n_ag * 7 * (N + 1) : 0, n_pu = plans ? n_ag * 2 * N : 0;      // without plans: reserved only
    const size_t n_pairs = n_ag * (M - 1), n_out = n_pairs * (POSE ? 3 : 2) * (N + 1), n_tv = n_pairs * 2;
    const T *dx, *da, *dpx, *dpu;
    const int32_t *dr, *dhp;
    T *dout, *dtv;
    Staging stg(h, mem, stream);
    stg.in(&dx, x, n_x); stg.in(&da, a_prev, n_ag); stg.in(&dr, route, n_ag);
    stg.in(&dhp, has_plan, n_ag, plans); stg.in(&dpx, plan_x, n_px); stg.in(&dpu, plan_u, n_pu);
    stg.out(&dout, obs_xy, n_out); stg.out(&dtv, tv_sv, n_tv);
    if (int rc = stg.upload()) return rc;
    if constexpr (POSE)
        HIPCHK(igt::launch_forecast_scene_pose(h->kp, E, h->d_routes, h->n_routes, h->d_heads, dx, da, dr, plans ? dpx : nullptr,
                                               plans ? dpu : nullptr, plans ? dhp : nullptr, dout, dtv, stg.stream()));
    else
        HIPCHK(igt::launch_forecast_scene<T>(h->kp, E, h->d_routes, h->n_routes, dx, da, dr, plans ? dpx : nullptr,
                                             plans ? dpu : nullptr, plans ? dhp : nullptr, dout, dtv, stg.stream()));
    return stg.download();
}

template <typename T>
int cartesian_impl(igt_handle* h, int32_t n, int32_t steps, const T* z0, const T* u, T* z_out, int mem, void* stream) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (n < 0 || steps < 0) return fail(IGT_E_INVALID, "negative size");
    if (n == 0) return IGT_OK;
    if (!z0 || !z_out || (steps > 0 && !u)) return fail(IGT_E_INVALID, "null buffer");
    const size_t n_z = (size_t)n * 4, n_u = (size_t)n * 2 * steps, n_o = (size_t)n * 4 * (steps + 1);
    const T *dz, *du;
    T* dout;
    Staging stg(h, mem, stream);
    stg.in(&dz, z0, n_z); stg.in(&du, u, n_u);      // steps == 0: u is reserved only
    stg.out(&dout, z_out, n_o);
    if (int rc = stg.upload()) return rc;
    HIPCHK(igt::launch_cartesian<T>(n, steps, h->p.dt, h->p.l_r, h->p.l_f, dz, du, dout, stg.stream()));
    return stg.download();
}

template <typename T>
int allgather_impl(igt_handle* h, int32_t B_local, const T* u_out, T* u0_all, void* stream) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (B_local < 0) return fail(IGT_E_INVALID, "B_local < 0");
    if (!h->comm) {         // no communicator = one shard: the gathered vector is the local one
        if (B_local == 0) return IGT_OK;
        if (!u_out || !u0_all) return fail(IGT_E_INVALID, "null buffer");
        HIPCHK(hipSetDevice(h->device));
        hipStream_t st0 = stream ? (hipStream_t)stream : h->stream;
        HIPCHK(igt::launch_first_controls<T>(B_local, h->p.N, u_out, u0_all, st0));
        return IGT_OK;
    }
    // With a communicator every rank enters ncclAllGather with the SAME count or the peers hang / read garbage: an
    // empty shard is refused (pad it, as the header says), and the count of the first call is the communicator's.
    if (B_local == 0) return fail(IGT_E_INVALID, "B_local == 0 with a communicator: every rank must take part with the same padded B_local");
    if (h->comm_B_local == 0) h->comm_B_local = B_local;
    else if (h->comm_B_local != B_local)
        return fail(IGT_E_INVALID, "B_local changed since the communicator's first all-gather (all ranks must pass one padded shard size)");
    if (!u_out || !u0_all) return fail(IGT_E_INVALID, "null buffer");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const size_t bytes = (size_t)B_local * 2 * sizeof(T);
    if (bytes > h->u0_bytes) {
        if (capturing(st)) return fail(IGT_E_STATE, "staging buffer too small for stream capture: run one eager call first");
        HIPCHK(hipStreamSynchronize(st));
        if (h->d_u0) { HIPCHK(hipFree(h->d_u0)); h->d_u0 = nullptr; h->u0_bytes = 0; }
        HIPCHK(hipMalloc(&h->d_u0, bytes + 256));
        h->u0_bytes = bytes;
    }
    HIPCHK(igt::launch_first_controls<T>(B_local, h->p.N, u_out, reinterpret_cast<T*>(h->d_u0), st));
    Rccl* r = rccl();
    if (int rc = r->AllGather(h->d_u0, u0_all, (size_t)B_local * 2, sizeof(T) == 4 ? 7 /* ncclFloat */ : 8 /* ncclDouble */,
                              h->comm, st))
        return rccl_fail(r, "ncclAllGather", rc);
    return IGT_OK;
}

}  // namespace

extern "C" {

int igt_version(void) { return IGT_VERSION; }

const char* igt_last_error(void) { return g_err.c_str(); }

int igt_params_default(igt_params* p) {
    if (!p) return fail(IGT_E_INVALID, "null params");
    std::memset(p, 0, sizeof(*p));
    p->N = 20; p->n_rk4 = 4; p->C = 256; p->n_obs = 1;
    p->cand_mode = IGT_CAND_LATTICE; p->cost_mode = IGT_COST_PROGRESS;
    p->dt = 0.1;
    p->l_r = 4.47 / 2; p->l_f = 4.47 / 2;                 /* mpc.py:48-50 */
    p->v_min = 0; p->v_max = 5; p->a_min = -4; p->a_max = 3; p->df_max = 1;  /* mpc.py:57-62 */
    p->jerk_limit = 0.9; p->steer_rate_limit = 0.7;       /* mpc.py:55-56 */
    p->ey_lim = 0.2;                                      /* mpc.py:61 */
    p->d_min = 2 * 2.8;                                   /* mpc.py:45, fourwayint.yaml:9 */
    p->w_u = 0.05;                                        /* mpc.py:362 */
    p->feas_tol = 1e-6;
    p->refine_iters = 0;
    p->polish_iters = 0;
    p->track_ke = 0.3; p->track_span = 0.1; p->track_beta_lim = 0.7; p->track_env = 1.0; p->track_vcap = 1.0;
    return IGT_OK;
}

int igt_create(const igt_params* p, int device, igt_handle** out) {
    if (!p || !out) return fail(IGT_E_INVALID, "null argument");
    std::string why;
    if (validate(*p, why)) return fail(IGT_E_INVALID, why);
#if !IGT_DEV_KERNELS
    if (const char* e = getenv("IGT_DEV_FLAGS"))
        if (atoi(e) & igt::DEV_KERNEL_FLAGS)
            return fail(IGT_E_INVALID, "IGT_DEV_FLAGS selects developer kernels (32 / 1024 / 2048) that this library is built without; "
                                       "load libigtmpc_dev.so (built with IGT_DEV_KERNELS=1)");
#endif
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(IGT_E_INVALID, "no such device");
    HIPCHK(hipSetDevice(device));
    igt_handle* h = new (std::nothrow) igt_handle();
    if (!h) return fail(IGT_E_NOMEM, "out of host memory");
    h->p = *p;
    h->kp = make_kp(*p, 0);
    h->device = device;
    // developer sweeps: the environment is read here, not on every solve
    if (const char* e = std::getenv("IGT_DEV_CKPT")) h->dev_ckpt = std::max(std::atoi(e), 0);
    if (const char* e = std::getenv("IGT_DEV_TRAJ_MAX")) h->dev_traj_max = std::max(std::atoi(e), 0);
    if (const char* e = std::getenv("IGT_DEV_POISON")) {      // a whole decimal number in 0..255; anything else is ignored
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == '\0' && v >= 0 && v <= 255) h->dev_poison = (int)v;
    }
#if IGT_DEV_KERNELS
    // sweeps of the slot reserve (igt_launch.h search64_grid): waves per 8 compute units a float64 search leaves alone
    if (const char* e = std::getenv("IGT_DEV_RESERVE")) h->dev_reserve_pool = std::max(std::atoi(e), 0);
    if (const char* e = std::getenv("IGT_DEV_RESERVE_UNITS")) h->dev_reserve_units = std::max(std::atoi(e), 0);
#endif
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) h->n_cu = v; }
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(IGT_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    for (int i = 0; i < 3; ++i) {
        e = hipEventCreate(&h->ev[i]);
        if (e != hipSuccess) { delete h; return fail(IGT_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
    }
    e = igt::prepare_emit_kernels();
    if (e != hipSuccess) { (void)igt_destroy(h); return fail(IGT_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e)); }
    *out = h;
    return IGT_OK;
}

int igt_destroy(igt_handle* h) {
    if (!h) return IGT_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->d_cinf) (void)hipFree(h->d_cinf);
    if (h->d_table) (void)hipFree(h->d_table);
    if (h->d_stage) (void)hipFree(h->d_stage);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->d_work) (void)hipFree(h->d_work);
    if (h->d_net) (void)hipFree(h->d_net);
    if (h->d_routes) (void)hipFree(h->d_routes);
    if (h->d_heads) (void)hipFree(h->d_heads);
    if (h->d_u0) (void)hipFree(h->d_u0);
    if (h->comm) { if (Rccl* r = rccl()) (void)r->CommDestroy(h->comm); h->comm = nullptr; rccl_release(); }
    for (int i = 0; i < 3; ++i) (void)hipEventDestroy(h->ev[i]);
    (void)hipStreamDestroy(h->stream);
    delete h;
    return IGT_OK;
}

int igt_get_params(const igt_handle* h, igt_params* out) {
    if (!h || !out) return fail(IGT_E_INVALID, "null argument");
    *out = h->p;
    return IGT_OK;
}

int igt_set_cinf(igt_handle* h, const double* A, const double* b, int32_t F) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (F < 0 || F > IGT_MAX_CINF) return fail(IGT_E_INVALID, "F must be in [0, IGT_MAX_CINF]");
    if (F > 0 && (!A || !b)) return fail(IGT_E_INVALID, "null table");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_cinf) { HIPCHK(hipFree(h->d_cinf)); h->d_cinf = nullptr; }
    if (F > 0) {
        std::vector<double> packed((size_t)F * 3);
        for (int m = 0; m < F; ++m) {
            packed[m * 3 + 0] = A[m * 2 + 0];
            packed[m * 3 + 1] = A[m * 2 + 1];
            packed[m * 3 + 2] = b[m];
        }
        HIPCHK(hipMalloc((void**)&h->d_cinf, packed.size() * sizeof(double)));
        HIPCHK(hipMemcpy(h->d_cinf, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    h->kp.F = F;
    return IGT_OK;
}

int igt_set_candidate_table(igt_handle* h, const double* U) {
    if (!h || !U) return fail(IGT_E_INVALID, "null argument");
    if (h->p.cand_mode != IGT_CAND_TABLE) return fail(IGT_E_STATE, "handle was not created with IGT_CAND_TABLE");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->p.C * 2 * h->p.N;
    if (!h->d_table) HIPCHK(hipMalloc((void**)&h->d_table, n * sizeof(double)));
    HIPCHK(hipMemcpy(h->d_table, U, n * sizeof(double), hipMemcpyHostToDevice));
    h->table_set = true;
    return IGT_OK;
}

int igt_set_value_net(igt_handle* h, int32_t n_layers, const int32_t* dims, const double* weights, const double* Wn,
                      const double* mu_f, double sigma_t, double mu_t) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (!dims || !weights || !Wn || !mu_f) return fail(IGT_E_INVALID, "null argument");
    if (n_layers != 3 && n_layers != 4) return fail(IGT_E_INVALID, "value net must have 2 or 3 hidden layers (3 or 4 Linear layers)");
    const int H = igt::VN_H;
    if (dims[0] != 6 || dims[n_layers] != 1) return fail(IGT_E_INVALID, "value net must map 6 -> 1");
    for (int l = 1; l < n_layers; ++l)
        if (dims[l] != H) return fail(IGT_E_INVALID, "hidden width must be 128");
    const int nm = n_layers - 2;   // hidden -> hidden matrices
    // unpack [W(out,in) row-major, b(out)] per layer
    const double* W1 = weights;                 // [H,6]
    const double* b1 = W1 + (size_t)H * 6;
    const double* Wh[2] = {nullptr, nullptr};
    const double* bh[2] = {nullptr, nullptr};
    const double* cur = b1 + H;
    for (int m = 0; m < nm; ++m) { Wh[m] = cur; bh[m] = cur + (size_t)H * H; cur = bh[m] + H; }
    const double* Wo = cur;                     // [1,H]
    const double bo = Wo[H];
    // host block: A1[H*6] c1[H] (WT[H*H] bias[H]) x nm, wout[H]
    const size_t n = (size_t)H * 6 + H + (size_t)nm * ((size_t)H * H + H) + H;
    std::vector<double> blk(n);
    double* A1 = blk.data();
    double* c1 = A1 + (size_t)H * 6;
    for (int i = 0; i < H; ++i) {
        double acc = b1[i];
        for (int k = 0; k < 6; ++k) {
            double a = 0.0;
            for (int j = 0; j < 6; ++j) a += W1[i * 6 + j] * Wn[j * 6 + k];     // A1 = W1 Wn
            A1[i * 6 + k] = a;
            acc -= a * mu_f[k];                                                 // c1 = b1 - A1 mu_f
        }
        c1[i] = acc;
    }
    double* q = c1 + H;
    size_t offWT[2] = {0, 0}, offB[2] = {0, 0};
    for (int m = 0; m < nm; ++m) {
        offWT[m] = (size_t)(q - blk.data());
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < H; ++j) q[(size_t)i * H + j] = Wh[m][(size_t)j * H + i];   // [i][j] = W[j][i]
        q += (size_t)H * H;
        offB[m] = (size_t)(q - blk.data());
        for (int j = 0; j < H; ++j) q[j] = bh[m][j];
        q += H;
    }
    const size_t offWo = (size_t)(q - blk.data());
    for (int j = 0; j < H; ++j) q[j] = Wo[j];
    // float block = the plain arrays followed by the MFMA fragment block (igt_value_net.h, value_mfma_kernel)
    const size_t nfrag = (size_t)igt::frag_floats(nm);
    std::vector<float> blkf(n + nfrag);
    for (size_t i = 0; i < n; ++i) blkf[i] = (float)blk[i];
    {
        float* f = blkf.data() + n;
        for (int t = 0; t < 4; ++t)                       // A1F: [A1 | c1 | 0] in A-operand order
            for (int s4 = 0; s4 < 4; ++s4)
                for (int l = 0; l < 64; ++l) {
                    const int i = 32 * t + (l & 31), k = 2 * s4 + (l >> 5);
                    *f++ = (float)(k < 6 ? A1[i * 6 + k] : (k == 6 ? c1[i] : 0.0));
                }
        for (int m = 0; m < nm; ++m)                      // WF[m]: W[j][i], i in the accumulator's row order
            for (int t = 0; t < 4; ++t)
                for (int ks = 0; ks < 64; ++ks)
                    for (int l = 0; l < 64; ++l) {
                        const int j = 32 * t + (l & 31), i = 32 * (ks >> 4) + igt::frag_row(ks & 15, l >> 5);
                        *f++ = (float)Wh[m][(size_t)j * H + i];
                    }
        for (int m = 0; m < nm; ++m)                      // BF[m]
            for (int t = 0; t < 4; ++t)
                for (int r = 0; r < 16; ++r)
                    for (int hh = 0; hh < 2; ++hh) *f++ = (float)bh[m][32 * t + igt::frag_row(r, hh)];
        for (int t = 0; t < 4; ++t)                       // WOF
            for (int r = 0; r < 16; ++r)
                for (int hh = 0; hh < 2; ++hh) *f++ = (float)Wo[32 * t + igt::frag_row(r, hh)];
    }
    // double block = the plain arrays followed by the f64 MFMA fragment block (igt_value_net.h, value_mfma_f64_kernel):
    // lane (i = l & 15, g = l >> 4) of k-step (T, r) holds W[16 To + i][16 T + 4 r + g]
    const size_t nfragd = (size_t)igt::fragd_doubles(nm);
    blk.resize(n + nfragd);
    A1 = blk.data(); c1 = A1 + (size_t)H * 6;            // (the resize may have moved the block)
    {
        double* f = blk.data() + n;
        for (int t = 0; t < 8; ++t)                       // A1F: [A1 | c1 | 0]
            for (int s2 = 0; s2 < 2; ++s2)
                for (int l = 0; l < 64; ++l) {
                    const int i = 16 * t + (l & 15), k = 4 * s2 + (l >> 4);
                    *f++ = k < 6 ? A1[i * 6 + k] : (k == 6 ? c1[i] : 0.0);
                }
        for (int m = 0; m < nm; ++m)                      // WF[m]
            for (int t = 0; t < 8; ++t)
                for (int ti = 0; ti < 8; ++ti)
                    for (int r = 0; r < 4; ++r)
                        for (int l = 0; l < 64; ++l)
                            *f++ = Wh[m][(size_t)(16 * t + (l & 15)) * H + (16 * ti + 4 * r + (l >> 4))];
        for (int m = 0; m < nm; ++m)                      // BF[m]: bias of row 16 t + g + 4 r
            for (int t = 0; t < 8; ++t)
                for (int r = 0; r < 4; ++r)
                    for (int g = 0; g < 4; ++g) *f++ = bh[m][16 * t + g + 4 * r];
        for (int t = 0; t < 8; ++t)                       // WOF
            for (int r = 0; r < 4; ++r)
                for (int g = 0; g < 4; ++g) *f++ = Wo[16 * t + g + 4 * r];
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_net) { HIPCHK(hipFree(h->d_net)); h->d_net = nullptr; }
    const size_t bytes_f = (((n + nfrag) * 4 + 255) / 256) * 256;
    HIPCHK(hipMalloc(&h->d_net, bytes_f + (n + nfragd) * 8));
    float* df = reinterpret_cast<float*>(h->d_net);
    double* dd = reinterpret_cast<double*>(reinterpret_cast<char*>(h->d_net) + bytes_f);
    HIPCHK(hipMemcpy(df, blkf.data(), (n + nfrag) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dd, blk.data(), (n + nfragd) * 8, hipMemcpyHostToDevice));
    auto fill = [&](auto& net, auto* base) {
        net.A1 = base; net.c1 = base + (size_t)H * 6;
        for (int m = 0; m < 2; ++m) { net.WT[m] = m < nm ? base + offWT[m] : nullptr; net.bias[m] = m < nm ? base + offB[m] : nullptr; }
        net.wout = base + offWo;
        net.n_hidden_mats = nm;
    };
    fill(h->net_f, df);
    fill(h->net_d, dd);
    h->net_f.frag = df + n; h->net_f.fragd = nullptr;
    h->net_d.frag = nullptr; h->net_d.fragd = dd + n;
    h->net_f.bout = (float)bo; h->net_f.sigma_t = (float)sigma_t; h->net_f.mu_t = (float)mu_t;
    h->net_d.bout = bo; h->net_d.sigma_t = sigma_t; h->net_d.mu_t = mu_t;
    HIPCHK(igt::prepare_value_kernels(nm));
    h->net_set = true;
    return IGT_OK;
}

int igt_solve_batch_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev, const float* kparams,
                        const uint32_t* flags, const float* obs_xy, const float* tv_sv, const float* enc, float* x_out,
                        float* u_out, float* cost_out, int32_t* argmin_out, int32_t* status_out, int mem, void* stream) {
    return solve_impl<float>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, nullptr, x_out, u_out, cost_out,
                             argmin_out, status_out, mem, stream);
}
int igt_solve_batch_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                        const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc,
                        double* x_out, double* u_out, double* cost_out, int32_t* argmin_out, int32_t* status_out,
                        int mem, void* stream) {
    return solve_impl<double>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, nullptr, x_out, u_out, cost_out,
                              argmin_out, status_out, mem, stream);
}
int igt_solve_batch_ws_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev, const float* kparams,
                           const uint32_t* flags, const float* obs_xy, const float* tv_sv, const float* enc,
                           const float* u_ws, float* x_out, float* u_out, float* cost_out, int32_t* argmin_out,
                           int32_t* status_out, int mem, void* stream) {
    return solve_impl<float>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, u_ws, x_out, u_out, cost_out,
                             argmin_out, status_out, mem, stream);
}
int igt_solve_batch_ws_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                           const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc,
                           const double* u_ws, double* x_out, double* u_out, double* cost_out, int32_t* argmin_out,
                           int32_t* status_out, int mem, void* stream) {
    return solve_impl<double>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, u_ws, x_out, u_out, cost_out,
                              argmin_out, status_out, mem, stream);
}

int igt_rollout_batch_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev, const float* kparams,
                          const uint32_t* flags, const float* obs_xy, const float* tv_sv, const float* enc,
                          float* X_all, float* U_all, float* cost_all, uint32_t* viol_all, int mem, void* stream) {
    return rollout_impl<float>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, nullptr, X_all, U_all, cost_all,
                               viol_all, mem, stream);
}
int igt_rollout_batch_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                          const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc,
                          double* X_all, double* U_all, double* cost_all, uint32_t* viol_all, int mem, void* stream) {
    return rollout_impl<double>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, nullptr, X_all, U_all, cost_all,
                                viol_all, mem, stream);
}
int igt_rollout_batch_ws_f32(igt_handle* h, int32_t B, const float* x0, const float* u_prev, const float* kparams,
                             const uint32_t* flags, const float* obs_xy, const float* tv_sv, const float* enc,
                             const float* u_ws, float* X_all, float* U_all, float* cost_all, uint32_t* viol_all, int mem,
                             void* stream) {
    return rollout_impl<float>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, u_ws, X_all, U_all, cost_all,
                               viol_all, mem, stream);
}
int igt_rollout_batch_ws_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                             const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc,
                             const double* u_ws, double* X_all, double* U_all, double* cost_all, uint32_t* viol_all,
                             int mem, void* stream) {
    return rollout_impl<double>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, u_ws, X_all, U_all, cost_all,
                                viol_all, mem, stream);
}

int igt_solve_candidates_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                             const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc, const double* U,
                             double* x_out, double* u_out, double* cost_out, int32_t* argmin_out, int32_t* status_out, int mem,
                             void* stream) {
    if (int rc = check_candidates(h, B, U)) return rc;
    return solve_impl<double>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, nullptr, x_out, u_out, cost_out, argmin_out,
                              status_out, mem, stream, U);
}
int igt_rollout_candidates_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                               const uint32_t* flags, const double* obs_xy, const double* tv_sv, const double* enc, const double* U,
                               double* X_all, double* U_all, double* cost_all, uint32_t* viol_all, int mem, void* stream) {
    if (int rc = check_candidates(h, B, U)) return rc;
    return rollout_impl<double>(h, B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, nullptr, X_all, U_all, cost_all, viol_all, mem,
                                stream, U);
}

int igt_solve_batch_box_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                            const uint32_t* flags, const double* obs_pose, const double* tv_sv, const double* enc,
                            const double* u_ws, double length, double width, double d_box, double* x_out, double* u_out,
                            double* cost_out, int32_t* argmin_out, int32_t* status_out, int mem, void* stream) {
    igt::BoxModel box;
    if (int rc = check_box(h, B, length, width, d_box, &box)) return rc;
    return solve_impl<double>(h, B, x0, u_prev, kparams, flags, obs_pose, tv_sv, enc, u_ws, x_out, u_out, cost_out, argmin_out,
                              status_out, mem, stream, nullptr, &box);
}
int igt_rollout_batch_box_f64(igt_handle* h, int32_t B, const double* x0, const double* u_prev, const double* kparams,
                              const uint32_t* flags, const double* obs_pose, const double* tv_sv, const double* enc,
                              const double* u_ws, double length, double width, double d_box, double* X_all, double* U_all,
                              double* cost_all, uint32_t* viol_all, int mem, void* stream) {
    igt::BoxModel box;
    if (int rc = check_box(h, B, length, width, d_box, &box)) return rc;
    return rollout_impl<double>(h, B, x0, u_prev, kparams, flags, obs_pose, tv_sv, enc, u_ws, X_all, U_all, cost_all, viol_all, mem,
                                stream, nullptr, &box);
}

int igt_frenet_step_f32(igt_handle* h, int32_t n, const float* x, const float* u, const float* kparams, float* x_next,
                        int mem, void* stream) {
    return frenet_step_impl<float>(h, n, x, u, kparams, x_next, mem, stream);
}
int igt_frenet_step_f64(igt_handle* h, int32_t n, const double* x, const double* u, const double* kparams,
                        double* x_next, int mem, void* stream) {
    return frenet_step_impl<double>(h, n, x, u, kparams, x_next, mem, stream);
}

int igt_set_routes(igt_handle* h, int32_t n_routes, const double* table) {
    if (!h || !table) return fail(IGT_E_INVALID, "null argument");
    if (n_routes < 1 || n_routes > 64) return fail(IGT_E_INVALID, "n_routes must be in [1, 64]");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_heads && n_routes != h->n_routes) { HIPCHK(hipFree(h->d_heads)); h->d_heads = nullptr; }      // headings of another table
    if (h->d_routes) { HIPCHK(hipFree(h->d_routes)); h->d_routes = nullptr; h->n_routes = 0; }
    HIPCHK(hipMalloc((void**)&h->d_routes, (size_t)n_routes * 12 * sizeof(double)));
    HIPCHK(hipMemcpy(h->d_routes, table, (size_t)n_routes * 12 * sizeof(double), hipMemcpyHostToDevice));
    h->n_routes = n_routes;
    return IGT_OK;
}

int igt_set_route_headings(igt_handle* h, int32_t n_routes, const double* table) {
    if (!h) return fail(IGT_E_INVALID, "igt_set_route_headings: null handle");
    if (!table) return fail(IGT_E_INVALID, "igt_set_route_headings: null table");
    if (!h->d_routes) return fail(IGT_E_INVALID, "igt_set_route_headings: route table not set (igt_set_routes first)");
    if (n_routes != h->n_routes)
        return fail(IGT_E_INVALID, "igt_set_route_headings: n_routes = " + std::to_string(n_routes) + " but the igt_set_routes table has " +
                                       std::to_string(h->n_routes) + " routes");
    for (int i = 0; i < n_routes; ++i)
        if (!std::isfinite(table[(size_t)i * 3 + 0]) || !std::isfinite(table[(size_t)i * 3 + 1]))
            return fail(IGT_E_INVALID, "igt_set_route_headings: h0 / hN of route " + std::to_string(i) + " is not finite");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!h->d_heads) HIPCHK(hipMalloc((void**)&h->d_heads, (size_t)n_routes * 3 * sizeof(double)));
    HIPCHK(hipMemcpy(h->d_heads, table, (size_t)n_routes * 3 * sizeof(double), hipMemcpyHostToDevice));
    return IGT_OK;
}

int igt_forecast_scene_pose_f64(igt_handle* h, int32_t E, const double* x, const double* a_prev, const int32_t* route,
                                const double* plan_x, const double* plan_u, const int32_t* has_plan, double* obs_pose,
                                double* tv_sv, int mem, void* stream) {
    return forecast_scene_impl<double, true>(h, E, x, a_prev, route, plan_x, plan_u, has_plan, obs_pose, tv_sv, mem, stream);
}
int igt_forecast_batch_pose_f64(igt_handle* h, int32_t B, const double* ego_xyh, const double* opp, const double* opp_a,
                                const int32_t* opp_route, const double* opp_heading, const double* plan_x, const double* plan_u,
                                const int32_t* has_plan, double* obs_pose, double* tv_sv, int mem, void* stream) {
    return forecast_impl<double, true>(h, B, ego_xyh, opp, opp_a, opp_route, opp_heading, plan_x, plan_u, has_plan, obs_pose, tv_sv,
                                       mem, stream);
}

int igt_forecast_batch_f32(igt_handle* h, int32_t B, const float* ego_xyh, const float* opp, const float* opp_a,
                           const int32_t* opp_route, const float* plan_x, const float* plan_u, const int32_t* has_plan,
                           float* obs_xy, float* tv_sv, int mem, void* stream) {
    return forecast_impl<float>(h, B, ego_xyh, opp, opp_a, opp_route, nullptr, plan_x, plan_u, has_plan, obs_xy, tv_sv, mem, stream);
}
int igt_loop_advance_f64(igt_handle* h, int32_t n, double* x, double* u_prev, const double* kparams, const int32_t* status,
                         const double* x_sol, const double* u_sol, double a_brake, int32_t* has_plan, double* plan_x,
                         double* plan_u, double* u_ws, const uint32_t* flags_in, uint32_t* flags_out, int64_t* infeasible,
                         double* x_log, double* u_log, const int64_t* step, int32_t T_log, int mem, void* stream) {
    return loop_advance_impl<double>(h, n, x, u_prev, kparams, status, x_sol, u_sol, a_brake, has_plan, plan_x, plan_u, u_ws,
                                     flags_in, flags_out, infeasible, x_log, u_log, step, T_log, mem, stream);
}
int igt_loop_advance_f32(igt_handle* h, int32_t n, double* x, double* u_prev, const double* kparams, const int32_t* status,
                         const float* x_sol, const float* u_sol, double a_brake, int32_t* has_plan, float* plan_x,
                         float* plan_u, float* u_ws, const uint32_t* flags_in, uint32_t* flags_out, int64_t* infeasible,
                         double* x_log, double* u_log, const int64_t* step, int32_t T_log, int mem, void* stream) {
    return loop_advance_impl<float>(h, n, x, u_prev, kparams, status, x_sol, u_sol, a_brake, has_plan, plan_x, plan_u, u_ws,
                                    flags_in, flags_out, infeasible, x_log, u_log, step, T_log, mem, stream);
}
int igt_forecast_scene_f32(igt_handle* h, int32_t E, const float* x, const float* a_prev, const int32_t* route,
                           const float* plan_x, const float* plan_u, const int32_t* has_plan, float* obs_xy, float* tv_sv,
                           int mem, void* stream) {
    return forecast_scene_impl<float>(h, E, x, a_prev, route, plan_x, plan_u, has_plan, obs_xy, tv_sv, mem, stream);
}
int igt_forecast_scene_f64(igt_handle* h, int32_t E, const double* x, const double* a_prev, const int32_t* route,
                           const double* plan_x, const double* plan_u, const int32_t* has_plan, double* obs_xy, double* tv_sv,
                           int mem, void* stream) {
    return forecast_scene_impl<double>(h, E, x, a_prev, route, plan_x, plan_u, has_plan, obs_xy, tv_sv, mem, stream);
}
int igt_forecast_batch_f64(igt_handle* h, int32_t B, const double* ego_xyh, const double* opp, const double* opp_a,
                           const int32_t* opp_route, const double* plan_x, const double* plan_u, const int32_t* has_plan,
                           double* obs_xy, double* tv_sv, int mem, void* stream) {
    return forecast_impl<double>(h, B, ego_xyh, opp, opp_a, opp_route, nullptr, plan_x, plan_u, has_plan, obs_xy, tv_sv, mem, stream);
}

int igt_cartesian_euler_f32(igt_handle* h, int32_t n, int32_t T, const float* z0, const float* u, float* z_out,
                            int mem, void* stream) {
    return cartesian_impl<float>(h, n, T, z0, u, z_out, mem, stream);
}
int igt_cartesian_euler_f64(igt_handle* h, int32_t n, int32_t T, const double* z0, const double* u, double* z_out,
                            int mem, void* stream) {
    return cartesian_impl<double>(h, n, T, z0, u, z_out, mem, stream);
}

int igt_comm_unique_id(void* id_out) {
    if (!id_out) return fail(IGT_E_INVALID, "null argument");
    Rccl* r = rccl_acquire();
    if (!r) return fail(IGT_E_STATE, "RCCL (librccl.so.1) could not be loaded");
    IgtNcclId id;
    const int rc = r->GetUniqueId(&id);
    const int ret = rc ? rccl_fail(r, "ncclGetUniqueId", rc) : IGT_OK;
    rccl_release();
    if (ret) return ret;
    std::memcpy(id_out, id.internal, IGT_COMM_ID_BYTES);
    return IGT_OK;
}

int igt_comm_init(igt_handle* h, int32_t world, int32_t rank, const void* id) {
    if (!h || !id) return fail(IGT_E_INVALID, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(IGT_E_INVALID, "need 0 <= rank < world");
    if (h->comm) return fail(IGT_E_STATE, "communicator already initialised (igt_comm_destroy first)");
    Rccl* r = rccl_acquire();          // held until igt_comm_destroy / igt_destroy
    if (!r) return fail(IGT_E_STATE, "RCCL (librccl.so.1) could not be loaded");
    if (hipError_t e = hipSetDevice(h->device)) { rccl_release(); return fail(IGT_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)); }
    IgtNcclId nid;
    std::memcpy(nid.internal, id, IGT_COMM_ID_BYTES);
    void* comm = nullptr;
    if (int rc = r->CommInitRank(&comm, world, nid, rank)) { const int ret = rccl_fail(r, "ncclCommInitRank", rc); rccl_release(); return ret; }
    h->comm = comm; h->comm_world = world; h->comm_rank = rank; h->comm_B_local = 0;
    return IGT_OK;
}

int igt_comm_destroy(igt_handle* h) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (!h->comm) return IGT_OK;
    Rccl* r = rccl();
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));          // no all-gather of this handle is still in flight on its own stream
    const int rc = r ? r->CommDestroy(h->comm) : 0;
    h->comm = nullptr; h->comm_world = 1; h->comm_rank = 0; h->comm_B_local = 0;
    const int ret = rc ? rccl_fail(r, "ncclCommDestroy", rc) : IGT_OK;
    rccl_release();                                   // the last communicator closes the binding
    return ret;
}


int igt_allgather_controls_f32(igt_handle* h, int32_t B_local, const float* u_out, float* u0_all, void* stream) {
    return allgather_impl<float>(h, B_local, u_out, u0_all, stream);
}
int igt_allgather_controls_f64(igt_handle* h, int32_t B_local, const double* u_out, double* u0_all, void* stream) {
    return allgather_impl<double>(h, B_local, u_out, u0_all, stream);
}

int igt_set_concurrency(igt_handle* h, int32_t solves_in_flight) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (solves_in_flight < 1 || solves_in_flight > 64) return fail(IGT_E_INVALID, "solves_in_flight must lie in [1, 64]");
    h->concurrency = solves_in_flight;
    return IGT_OK;
}

int igt_set_polish_gradient(igt_handle* h, int mode) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (mode != IGT_GRAD_FORWARD_DIFF && mode != IGT_GRAD_ADJOINT)
        return fail(IGT_E_INVALID, "mode must be IGT_GRAD_FORWARD_DIFF or IGT_GRAD_ADJOINT");
    h->polish_grad = mode;
    return IGT_OK;
}

int igt_set_polish_step(igt_handle* h, int mode) {
    if (mode != IGT_POLISH_STEP_GRADIENT && mode != IGT_POLISH_STEP_NEWTON)
        return fail(IGT_E_INVALID, "mode must be IGT_POLISH_STEP_GRADIENT or IGT_POLISH_STEP_NEWTON");
    if (!h) return fail(IGT_E_INVALID, "null handle (igt_set_polish_step: IGT_POLISH_STEP_GRADIENT or IGT_POLISH_STEP_NEWTON)");
    h->polish_step = mode;
    return IGT_OK;
}

int igt_set_value_polish(igt_handle* h, int iters) {
    if (!h) return fail(IGT_E_INVALID, "null handle (igt_set_value_polish)");
    if (iters < 0 || iters > igt::VALUE_POLISH_MAX_ITERS) return fail(IGT_E_INVALID, "igt_set_value_polish: iters must be in [0, 4]");
    if (h->p.cost_mode != IGT_COST_VALUE_NET)
        return fail(IGT_E_INVALID, "igt_set_value_polish needs a handle created with IGT_COST_VALUE_NET (the progress cost has polish_iters)");
    h->value_polish = iters;
    return IGT_OK;
}

int igt_cost_gradient_f64(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags,
                          const double* U, double* cost_out, double* grad_out, int mem, void* stream) {
    return cost_gradient_impl(h, B, x0, kparams, flags, U, cost_out, grad_out, mem, stream);
}

int igt_terminal_value_f64(igt_handle* h, int32_t n, const double* sv, const double* tv_sv, const double* enc, double* V_out,
                           double* dV_out, int mem, void* stream) {
    return terminal_value_impl(h, n, sv, tv_sv, enc, V_out, dV_out, mem, stream);
}

int igt_cost_gradient_vn_f64(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags,
                             const double* tv_sv, const double* enc, const double* U, double* cost_out, double* grad_out,
                             int mem, void* stream) {
    return cost_gradient_vn_impl(h, B, x0, kparams, flags, tv_sv, enc, U, cost_out, grad_out, mem, stream);
}

int igt_set_profiling(igt_handle* h, int enable) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    h->prof = enable != 0;
    h->ev_recorded = false;
    return IGT_OK;
}

int igt_get_kernel_ms(igt_handle* h, float* search_ms, float* emit_ms) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (!h->prof || !h->ev_recorded) return fail(IGT_E_STATE, "no profiled solve recorded");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->ev[2]));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
    if (search_ms) *search_ms = a;
    if (emit_ms) *emit_ms = b;
    return IGT_OK;
}

int igt_algorithmic_bytes_per_solve(const igt_handle* h, int elem_size, int64_t* read_bytes, int64_t* write_bytes) {
    if (!h) return fail(IGT_E_INVALID, "null handle");
    if (elem_size != 4 && elem_size != 8) return fail(IGT_E_INVALID, "elem_size must be 4 or 8");
    const igt_params& p = h->p;
    int64_t r = (int64_t)(7 + 2 + 3) * elem_size + 4 + (int64_t)p.n_obs * 2 * (p.N + 1) * elem_size;
    if (p.cost_mode == IGT_COST_VALUE_NET) r += 4 * elem_size;
    const int64_t w = (int64_t)(7 * (p.N + 1) + 2 * p.N) * elem_size + elem_size + 4 + 4;
    if (read_bytes) *read_bytes = r;
    if (write_bytes) *write_bytes = w;
    return IGT_OK;
}

}  // extern "C"
