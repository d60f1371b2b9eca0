#!/usr/bin/env python3
"""Developer probe (GPU box) for scenes of M vehicles; every call is one configuration in a fresh process.

    python tools/scene_loop_bench.py forecast M PROBLEMS    scene-major forecast against the gathered path (torch gathers +
                                                            igt_forecast_batch_f64), f64, N = 20, HIP events, bytes moved
    python tools/scene_loop_bench.py loop M PROBLEMS [PKG]  step time of the device-resident loop (eager and graph), N = 20, 50
                                                            steps; PKG = another checkout's igt-mpc-int_amd (e.g. the parent
                                                            commit's, M = 2 only there) for runs that take turns on one box
    python tools/scene_loop_bench.py quality M N            8 scenarios x 64 episodes, drivers' default: infeasible steps,
                                                            deadlock flag, mean final s
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode, M, arg = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
pkg = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'igt-mpc-int_amd')
sys.path.insert(0, pkg)
import numpy as np  # noqa: E402


def events_ms(fn, reps=200, warm=20):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):                       # five blocks: median and spread
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


if mode == 'forecast':
    import torch
    import igtmpc
    N, E = 20, max(1, arg // M)
    rng = np.random.default_rng(1)
    dev = lambda v: torch.as_tensor(v, device='cuda')
    x = dev(rng.uniform(0, 40, (E, M, 7)))
    a = dev(rng.uniform(-1, 1, (E, M)))
    rid = dev(rng.integers(0, 12, (E, M)).astype(np.int32))
    px, pu = dev(rng.uniform(0, 40, (E, M, 7, N + 1))), dev(rng.uniform(-1, 1, (E, M, 2, N)))
    hp = dev(rng.integers(0, 2, (E, M)).astype(np.int32))
    idx = dev(np.array([[j for j in range(M) if j != i] for i in range(M)]).reshape(-1))
    ix, io = dev(np.array([0, 1, 6])), dev(np.array([0, 1, 2, 5]))
    s = igtmpc.BatchSolver(N=N, n_obs=M - 1, dtype='f64')
    sq = (lambda v: v.squeeze(1)) if M == 2 else (lambda v: v)

    def gathered():
        g = lambda v: sq(v.index_select(1, idx).reshape((E * M, M - 1) + tuple(v.shape[2:]))).contiguous()
        return s.forecast(x.index_select(2, ix).reshape(E * M, 3).contiguous(), g(x.index_select(2, io)), g(a), g(rid), g(px),
                          g(pu), g(hp))

    scene = lambda: s.forecast_scene(x, a, rid, px, pu, hp)
    o1, o2 = gathered()[0], scene()[0]
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)
    out_b = E * M * (M - 1) * (2 * (N + 1) + 2) * 8
    in_b = E * M * (7 + 1 + 7 * (N + 1) + 2 * N) * 8 + 2 * E * M * 4
    gath_b = E * M * (M - 1) * (4 + 1 + 7 * (N + 1) + 2 * N) * 8 + E * M * 3 * 8          # written by the gathers, read again
    tg, ts = events_ms(gathered), events_ms(scene)
    print(json.dumps(dict(mode=mode, M=M, problems=E * M, gathered_ms=[round(v, 4) for v in tg], scene_ms=[round(v, 4) for v in ts],
                          scene_bytes=in_b + out_b, gathered_bytes=in_b + 2 * gath_b + out_b)), flush=True)
elif mode == 'loop':
    from igtmpc.evaluate import run_closed_loop
    E, steps = max(1, arg // M), 50
    kw = dict(sc=1, num_samples=E, N=20, T_sim=steps / 10, device_resident=True, **(dict(num_agents=M) if M != 2 else {}))
    row = dict(mode=mode, M=M, problems=E * M, pkg=os.path.relpath(pkg, ROOT))
    for name, g in (('eager', False), ('graph', True)):
        run_closed_loop(graph=g, **kw)                                           # warm-up (first-touch costs)
        ts = [run_closed_loop(graph=g, **kw)['wall_s'] / steps * 1e3 for _ in range(5)]
        row[f'{name}_ms_per_step'] = [round(float(v), 4) for v in (np.median(ts), min(ts), max(ts))]
    print(json.dumps(row), flush=True)
elif mode == 'quality':
    from igtmpc.evaluate import run_closed_loop
    N, inf, dl, fs = arg, [], [], []
    for sc in range(1, 9):
        r = run_closed_loop(sc=sc, num_samples=64, N=N, device_resident=True, **(dict(num_agents=M) if M != 2 else {}))
        inf.append(r['infeasible_ratio'].mean())
        dl.append(r['deadlock'].mean())
        fs.append(r['x_data'][:, 2::7, -1].mean())
    print(json.dumps(dict(mode=mode, M=M, N=N, infeasible_steps=round(float(np.mean(inf)), 4), deadlock_flag=round(float(np.mean(dl)), 4),
                          mean_final_s=round(float(np.mean(fs)), 2))), flush=True)
