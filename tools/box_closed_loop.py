"""Closed loop, N = 40, 512 episodes, same seed: 'circle' against 'obca' (host loop)."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'igt-mpc-int_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
import numpy as np
import box_collision_restated as R
from igtmpc.evaluate import run_closed_loop

for sc in range(1, 9):
    for ca in ('circle', 'obca'):
        t0 = time.time()
        r = run_closed_loop(sc=sc, num_samples=512, N=40, ca_type=ca, seed=2026)
        xd = r['x_data']                                    # [E, 14, T+1]
        a, b = xd[:, 0:7], xd[:, 7:14]
        gap = R.signed_gap(a[:, 0], a[:, 1], a[:, 6], b[:, 0], b[:, 1], b[:, 6])
        dist = np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1])
        prog = (xd[:, 2::7, -1] - xd[:, 2::7, 0]).mean()
        print(f'sc{sc} {ca:6s}: infeasible steps {100 * r["infeasible_ratio"].mean():.2f} %  deadlock flag {100 * r["deadlock"].mean():.2f} %  '
              f'progress {prog:.2f} m  smallest signed gap of the actual rectangles {gap.min():.4f} m  (episodes with gap < 0: '
              f'{int((gap.min(axis=1) < 0).sum())})  smallest centre distance {dist.min():.3f} m  solve {np.median(r["solve_ms"]):.3f} ms/step (host call, median)  '
              f'wall {time.time() - t0:.1f} s', flush=True)
