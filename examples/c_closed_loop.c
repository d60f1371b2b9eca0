/* c_closed_loop.c -- a closed loop on the C ABI of libigtmpc.so from plain C99: no Python, no torch.
 *
 * The time loop of the reference's evaluate.py (--eval_mode mpc, evaluate.py:451-564) for E scenes of M vehicles in lock-step,
 * T steps of
 *     igt_forecast_scene_f64  ->  igt_solve_batch_ws_f64  ->  igt_loop_advance_f64
 * through include/igtmpc.h alone.  Every buffer is a host array (IGT_MEM_HOST throughout): device buffers would need the HIP
 * runtime's headers, which a C99 compiler does not take without the platform's defines, so linking is kept as simple as
 * c_caller's.  A C++ or HIP caller passes hipMalloc'ed pointers and IGT_MEM_DEVICE to the same three calls and gets the
 * same bytes ("Streams, graphs, threads").
 *
 *   gcc -std=c99 -O2 -Iinclude examples/c_closed_loop.c -o c_closed_loop -Ligt-mpc-int_amd/igtmpc -ligtmpc \
 *       -Wl,-rpath,$PWD/igt-mpc-int_amd/igtmpc -L/opt/rocm/lib -lamdhip64 -lm
 *   ./c_closed_loop in.bin out.bin
 *
 * in.bin (native byte order, no padding):
 *   int32  E, M, N, T, n_routes, cand_mode (IGT_CAND_*), F, warm (0 / 1: pass the shifted plan as the warm start)
 *   double dt, track_env, a_brake, u_prev0[2]          (track_env is read with IGT_CAND_TRACK only; a_brake: mpc.yaml:8, -4)
 *   double routes[n_routes][12]                        (igt_set_routes)
 *   double cinf_A[F][2], cinf_b[F]                     (igt_set_cinf; F = 0: no terminal set)
 *   int32  route[E M]    double x0[E M][7]    uint32 flags[E M]    double kparams[E M][3]
 * out.bin:
 *   double x_log[E M][7][T+1], u_log[E M][2][T]        (the reference driver's cl_traj [E,7M,T+1] and u_cl [E,2M,T])
 *   int64  infeasible[E M]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "igtmpc.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != IGT_OK) {                                                     \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, igt_last_error());     \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static void* take(FILE* f, size_t count, size_t size) {
    void* p = malloc(count > 0 ? count * size : 1);
    if (!p || fread(p, size, count, f) != count) {
        fprintf(stderr, "short input file\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t* hd = take(f, 8, sizeof(int32_t));
    const int E = hd[0], M = hd[1], N = hd[2], T = hd[3], n_routes = hd[4], cand_mode = hd[5], F = hd[6], warm = hd[7];
    if (E < 1 || M < 2 || M > IGT_MAX_OBS + 1 || N < 1 || N > IGT_MAX_N || T < 1 || n_routes < 1 || F < 0 || F > IGT_MAX_CINF) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t n = (size_t)E * M;
    double* sc = take(f, 5, sizeof(double));
    const double dt = sc[0], track_env = sc[1], a_brake = sc[2];
    double* routes = take(f, (size_t)n_routes * 12, sizeof(double));
    double* cinf_A = take(f, (size_t)F * 2, sizeof(double));
    double* cinf_b = take(f, (size_t)F, sizeof(double));
    int32_t* route = take(f, n, sizeof(int32_t));
    double* x = take(f, n * 7, sizeof(double));                     /* the state, advanced in place */
    uint32_t* flags = take(f, n, sizeof(uint32_t));
    double* kparams = take(f, n * 3, sizeof(double));
    fclose(f);

    igt_params p;
    CHECK(igt_params_default(&p));                                   /* mpc.py:45-62 constants */
    p.N = N; p.dt = dt; p.n_obs = M - 1; p.cand_mode = cand_mode;
    if (cand_mode == IGT_CAND_TRACK) p.track_env = track_env;
    igt_handle* h = NULL;
    CHECK(igt_create(&p, 0, &h));
    CHECK(igt_set_routes(h, n_routes, routes));
    if (F > 0) CHECK(igt_set_cinf(h, cinf_A, cinf_b, F));

    const size_t n_sx = n * 7 * (size_t)(N + 1), n_su = n * 2 * (size_t)N, n_obs = n * (size_t)(M - 1) * 2 * (size_t)(N + 1);
    double* u_prev = malloc(n * 2 * sizeof(double));
    double* a_prev = malloc(n * sizeof(double));
    double* obs = malloc(n_obs * sizeof(double));
    double* tv = malloc(n * (size_t)(M - 1) * 2 * sizeof(double));
    double* x_sol = malloc(n_sx * sizeof(double));
    double* u_sol = malloc(n_su * sizeof(double));
    double* cost = malloc(n * sizeof(double));
    int32_t* argmin = malloc(n * sizeof(int32_t));
    int32_t* status = malloc(n * sizeof(int32_t));
    int32_t* has_plan = calloc(n, sizeof(int32_t));                 /* nobody has a plan before the first solve */
    double* plan_x = calloc(n_sx, sizeof(double));
    double* plan_u = calloc(n_su, sizeof(double));
    double* u_ws = calloc(n_su, sizeof(double));
    uint32_t* flags_ws = calloc(n, sizeof(uint32_t));
    int64_t* infeasible = calloc(n, sizeof(int64_t));
    double* x_log = calloc(n * 7 * (size_t)(T + 1), sizeof(double));
    double* u_log = calloc(n * 2 * (size_t)T, sizeof(double));
    if (!u_prev || !a_prev || !obs || !tv || !x_sol || !u_sol || !cost || !argmin || !status || !has_plan || !plan_x || !plan_u ||
        !u_ws || !flags_ws || !infeasible || !x_log || !u_log)
        return 2;
    for (size_t i = 0; i < n; ++i) {
        u_prev[i * 2 + 0] = sc[3];                                   /* evaluate.py:419: (0.1, 0) */
        u_prev[i * 2 + 1] = sc[4];
    }
    for (size_t r = 0; r < n * 7; ++r) x_log[r * (size_t)(T + 1)] = x[r];

    for (int64_t t = 0; t < T; ++t) {
        /* predict -> share motion forecasts -> filter_preds, for every (scene, ego) problem       (evaluate.py:455-477) */
        for (size_t i = 0; i < n; ++i) a_prev[i] = u_prev[i * 2];
        CHECK(igt_forecast_scene_f64(h, E, x, a_prev, route, plan_x, plan_u, has_plan, obs, tv, IGT_MEM_HOST, NULL));
        /* every problem at once; from the second step on an agent that solved passes its shifted plan  (evaluate.py:478-482) */
        const int ws = warm && t > 0;
        CHECK(igt_solve_batch_ws_f64(h, (int32_t)n, x, u_prev, kparams, ws ? flags_ws : flags, obs, NULL, NULL, ws ? u_ws : NULL,
                                     x_sol, u_sol, cost, argmin, status, IGT_MEM_HOST, NULL));
        /* apply or brake, share, shift, count, log                                                   (evaluate.py:491-545) */
        CHECK(igt_loop_advance_f64(h, (int32_t)n, x, u_prev, kparams, status, x_sol, u_sol, a_brake, has_plan, plan_x, plan_u,
                                   u_ws, flags, flags_ws, infeasible, x_log, u_log, &t, T, IGT_MEM_HOST, NULL));
    }
    CHECK(igt_destroy(h));

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    int bad = fwrite(x_log, sizeof(double), n * 7 * (size_t)(T + 1), f) != n * 7 * (size_t)(T + 1);
    bad |= fwrite(u_log, sizeof(double), n * 2 * (size_t)T, f) != n * 2 * (size_t)T;
    bad |= fwrite(infeasible, sizeof(int64_t), n, f) != n;
    bad |= fclose(f) != 0;
    long fallbacks = 0;
    for (size_t i = 0; i < n; ++i) fallbacks += (long)infeasible[i];
    printf("%d scenes of %d vehicles, %d steps: %ld fallback steps of %ld\n", E, M, T, fallbacks, (long)n * T);
    free(hd); free(sc); free(routes); free(cinf_A); free(cinf_b); free(route); free(x); free(flags); free(kparams);
    free(u_prev); free(a_prev); free(obs); free(tv); free(x_sol); free(u_sol); free(cost); free(argmin); free(status);
    free(has_plan); free(plan_x); free(plan_u); free(u_ws); free(flags_ws); free(infeasible); free(x_log); free(u_log);
    return bad ? 3 : 0;
}
