"""Rectangle (OBCA) closed loop: what a step costs with the pose forecast on the host and on the device (profiles/
pose_forecast_time.txt).  ca_type='obca', N = 40, E = 256 scenes of M = 2, tracking family, f64, sc 1:
    host loop, pose_forecast='host'    (the parent commit's path)
    host loop, pose_forecast='device'
    device-resident, step='torch'
    device-resident, step='fused'
    device-resident, step='fused', graph=True
One warm-up run each, then --runs alternating rounds.  Per run: ms per step = wall_s / steps for the device-resident loops (the
loop ends in a device synchronise), sum(solve_ms) / steps for the host loops (the solve call synchronises), and for all five the
whole call over its steps (set-up, tables and the result's copies included).

    python tools/pose_forecast_time.py [--runs 3] [--E 256] [--N 40] [--T_sim 15]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pose_forecast_time.py --trace
    python tools/pose_forecast_time.py --summarise DIR
--trace: one eager device-resident run with rectangles (the pose kernel) and one with circles (forecast_scene_kernel) at the same
E, N, for a kernel trace; --summarise prints the two kernels' rows of the trace's statistics."""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'igt-mpc-int_amd')]

CONFIGS = [('host loop, host pose', dict(pose_forecast='host')),
           ('host loop, device pose', dict(pose_forecast='device')),
           ('device-resident, torch step', dict(pose_forecast='device', device_resident=True, step='torch')),
           ('device-resident, fused step', dict(pose_forecast='device', device_resident=True, step='fused')),
           ('device-resident, fused + graph', dict(pose_forecast='device', device_resident=True, step='fused', graph=True))]


def summarise(d):
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit(f'no *kernel_stats.csv under {d}')
    for f in files:
        rows = list(csv.DictReader(open(f)))
        print(f'{os.path.relpath(f, d)}: {len(rows)} kernels; name, calls, mean / min / max us')
        for r in rows:
            if 'forecast' in r['Name'] or rows.index(r) < 4:
                print(f"  {r['Name'][:90]:90s} {int(r['Calls']):6d}  {float(r['AverageNs']) / 1e3:8.2f} {float(r['MinNs']) / 1e3:8.2f} "
                      f"{float(r['MaxNs']) / 1e3:8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--E', type=int, default=256)
    ap.add_argument('--N', type=int, default=40)
    ap.add_argument('--T_sim', type=float, default=15.0)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--summarise', default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import numpy as np
    import torch
    from igtmpc.evaluate import run_closed_loop
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured')
    kw = dict(sc=1, num_samples=a.E, N=a.N, cand_mode='track', dtype='f64')
    if a.trace:
        run_closed_loop(ca_type='obca', pose_forecast='device', device_resident=True, T_sim=5.0, **kw)
        run_closed_loop(ca_type='circle', device_resident=True, T_sim=5.0, **kw)
        return
    steps = int(round(a.T_sim / 0.1))

    def one(extra, T_sim):
        t0 = time.perf_counter()
        r = run_closed_loop(ca_type='obca', T_sim=T_sim, **kw, **extra)
        call = time.perf_counter() - t0
        n = r['x_data'].shape[2] - 1
        loop = r['wall_s'] if 'wall_s' in r else float(np.sum(r['solve_ms'])) / 1e3
        return loop / n * 1e3, call / n * 1e3, r

    ref = None
    for name, extra in CONFIGS:                      # warm-up: every shape the timed window uses
        one(extra, 1.0)
    res = {name: [] for name, _ in CONFIGS}
    for _ in range(a.runs):
        for name, extra in CONFIGS:
            loop, call, r = one(extra, a.T_sim)
            res[name].append((loop, call))
            if name == CONFIGS[1][0]:
                ref = r
            elif ref is not None and extra.get('pose_forecast') == 'device':
                assert all(np.array_equal(r[k], ref[k]) for k in ('x_data', 'u_data', 'infeasible_ratio')), name
    print(f'E = {a.E} scenes of 2, N = {a.N}, {steps} steps, tracking family, f64; ms per step, {a.runs} alternating runs')
    for name, _ in CONFIGS:
        lp, cl = [v[0] for v in res[name]], [v[1] for v in res[name]]
        print(f'  {name:32s} loop ' + ' '.join(f'{v:7.3f}' for v in lp) + f'  median {np.median(lp):7.3f}  spread '
              f'{(max(lp) - min(lp)) / np.median(lp) * 100:4.1f} %   | whole call ' + ' '.join(f'{v:7.3f}' for v in cl), flush=True)
    inf = ref['infeasible_ratio'].mean() * 100
    print(f'  device-pose runs byte-equal to each other (asserted); infeasible steps {inf:.2f} %, deadlock flag '
          f'{ref["deadlock"].mean() * 100:.2f} %')


if __name__ == '__main__':
    main()
