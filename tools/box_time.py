"""solve_box against solve on one handle: B = 4096, C = 256, N = 20, lattice and track; obstacles near (the benchmark batch's own
forecasts, heading along their motion) and all beyond the gate.  Device tensors, device events, alternating rounds."""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'igt-mpc-int_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
import numpy as np
import torch
import igtmpc
from igtmpc.scenarios import make_batch
from igtmpc.cinf import cinf_halfplanes

B, C, N = 4096, 256, 20
b = make_batch(B, dtype=np.float64, N=N)
obs = b['obs_xy']
d = np.diff(obs, axis=-1)
head = np.arctan2(d[:, :, 1], d[:, :, 0]); head = np.concatenate([head, head[..., -1:]], -1)
still = (np.abs(d).sum(axis=2) < 1e-9); still = np.concatenate([still, still[..., -1:]], -1)
head = np.where(still, 0.0, head)
near = np.ascontiguousarray(np.concatenate([obs, head[:, :, None, :]], axis=2))
far = near.copy(); far[:, :, 0] = b['x0'][:, 0, None, None] - 500.0; far[:, :, 1] = b['x0'][:, 1, None, None]
far_xy = np.ascontiguousarray(far[:, :, :2])
dev = lambda a: torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()
pos = [dev(b[k]) for k in ('x0', 'u_prev', 'kparams', 'flags')]
t_obs, t_near, t_far, t_far_xy = dev(obs), dev(near), dev(far), dev(far_xy)


def timed(fn, reps=100, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for cand in ('lattice', 'track'):
    with igtmpc.BatchSolver(N=N, C=C, n_obs=1, dtype='f64', cand_mode=cand) as s:
        s.set_cinf(*cinf_halfplanes())
        out = s.solve(*pos, t_obs)
        runs = dict(circle_near=lambda: s.solve(*pos, t_obs, out=out), box_near=lambda: s.solve_box(*pos, t_near, out=out),
                    circle_far=lambda: s.solve(*pos, t_far_xy, out=out), box_far=lambda: s.solve_box(*pos, t_far, out=out))
        res = {k: [] for k in runs}
        for r in range(3):
            for k, fn in runs.items():
                res[k].append(timed(fn))
        st = {}
        for k, fn in runs.items():
            fn(); torch.cuda.synchronize(); st[k] = int((out['status'] == 0).sum())
        for k in runs:
            print(f'{cand:8s} {k:12s} ms/solve ' + ' '.join(f'{v:.4f}' for v in res[k]) + f'   median {np.median(res[k]):.4f}   solved {st[k]}/{B}', flush=True)
