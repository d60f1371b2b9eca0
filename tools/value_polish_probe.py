"""Developer probe (not read by bench.py): what the polish under the value-network cost costs and what it buys, with either driver
(BatchSolver(value_polish_iters=, value_polish_driver=)): --driver host, the steps driven from numpy (igtmpc/solver.py
_value_polish_host; the default), or --driver device, the library's own loop inside the solve (igtmpc.h igt_set_value_polish).

--time: wall time of a host-mode gt_mpc solve (numpy arrays in, synchronised results out) with value_polish_iters 0 / 1 / 2 / 4 at
B = 1 (the planner's problem), 64, 256 and 1024, N = 20, V_GT_sc1 lattice and tracking and V_GT_sc3 lattice: median of --reps
solves after one warm-up, the extra time per solved scenario and iteration, and the mean drop of the cost over the solved scenarios.
--loop: run_closed_loop in gt_mpc (host loop), --episodes episodes, N = 20, with value_polish_iters 0 and 1: infeasible steps,
deadlock flag, mean final s and the mean solve time per step.
--cases sc:family,... and --sizes B,... cut --time down (the host driver takes 0.5 ms per solved scenario and iteration); --table
prints the --time rows as the table of profiles/value_polish_*_time.txt.
   python tools/value_polish_probe.py --driver device --time --loop [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'igt-mpc-int_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--episodes', type=int, default=512)
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--loop', action='store_true')
    ap.add_argument('--driver', choices=('host', 'device'), default='host')
    ap.add_argument('--cases', default='1:lattice,1:track,3:lattice')
    ap.add_argument('--sizes', default='1,64,256,1024')
    ap.add_argument('--table', action='store_true')
    args = ap.parse_args()
    import igtmpc
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.scenarios import make_batch
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.time:
        for sc, cand in [(int(c.split(':')[0]), c.split(':')[1]) for c in args.cases.split(',')]:
            net = igtmpc.shipped_value_net(sc)
            for B in [int(x) for x in args.sizes.split(',')]:
                b = make_batch(max(B, 64), N=20, dtype=np.float64)
                lo = 2 if B == 1 else 0
                a = [np.ascontiguousarray(b[k][lo:lo + B]) for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc')]
                with igtmpc.BatchSolver(dtype='f64', N=20, cost_mode='value_net', cand_mode=cand, value_polish_driver=args.driver) as s:
                    s.set_cinf(*cinf_halfplanes())
                    s.set_value_net(net['layers'])
                    base_ms = base_cost = None
                    for k in (0, 1, 2, 4):
                        s.set_value_polish(k)
                        out = s.solve(*a)
                        ts = []
                        for _ in range(args.reps):
                            t0 = time.perf_counter()
                            out = s.solve(*a)
                            ts.append((time.perf_counter() - t0) * 1e3)
                        ms = sorted(ts)[len(ts) // 2]
                        ok = out['status'] == 0
                        if k == 0:
                            base_ms, base_cost = ms, out['cost'].copy()
                        emit(dict(what='host-mode solve', driver=args.driver, net=f'V_GT_sc{sc}', cand=cand, B=B, solved=int(ok.sum()), iters=k,
                                  ms_median=round(ms, 3), ms_min=round(min(ts), 3),
                                  extra_us_per_solved_scenario_and_iteration=(round((ms - base_ms) * 1e3 / max(1, ok.sum()) / k, 1)
                                                                             if k else None),
                                  mean_cost_drop=float((base_cost[ok] - out['cost'][ok]).mean()) if ok.any() else None))
    if args.loop:
        from igtmpc.evaluate import run_closed_loop
        for k in (0, 1):
            t0 = time.perf_counter()
            r = run_closed_loop(sc=1, num_samples=args.episodes, N=20, eval_mode='gt_mpc', value_polish_iters=k,
                                value_polish_driver=args.driver)
            emit(dict(what='closed loop gt_mpc sc1 N=20 (host loop, shipped network, identity normalisation)', driver=args.driver,
                      episodes=args.episodes,
                      value_polish_iters=k, infeasible_steps=float(np.mean(r['infeasible_ratio'])),
                      deadlock_flag=float(np.mean(r['deadlock'])), mean_final_s=float(r['x_data'][:, 2::7, -1].mean()),
                      wall_s=round(time.perf_counter() - t0, 1)))
    if args.table:
        print('net      family        B  solved  k   ms/solve  extra us  mean cost drop')
        for r in rows:
            if r['what'] == 'host-mode solve':
                x = r['extra_us_per_solved_scenario_and_iteration']
                print(f"{r['net']:8s} {r['cand']:8s} {r['B']:6d} {r['solved']:7d} {r['iters']:2d} {r['ms_median']:10.3f} "
                      f"{'' if x is None else format(x, '9.1f'):>9s} {r['mean_cost_drop'] or 0.0:15.4f}", flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
