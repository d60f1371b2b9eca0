#!/usr/bin/env python3
"""Developer probe (GPU box): what per-scenario candidate sets cost.  One solve at a time, f64, progress cost, device tensors,
HIP events around each solve, 5 warm-up and 20 timed steps; B = 4096 with C = 256 and C = 64, N = 20:
  (a) solve_candidates on U[B,C,2,N];
  (b) solve on a table handle whose shared table is U[0]: the same arithmetic on an L2-resident table, the kernels the table
      family had before the entry -- the yardstick;
  (c) the streaming floor: the bytes of U over the HBM bandwidth bench.py uses for its roofline;
  (d) beside the three: solve_candidates on U[0] repeated for every scenario -- (b)'s candidates, so (b)'s roll-outs, early exits
      and answers, streamed from HBM instead of read from one L2-resident table.  (b) judges scenario 0's ramps against every
      other scenario's u_prev, where nearly all of them break the rate limit at step 0 and the units leave at once: (a) and (b)
      do not roll the same work, (d) and (b) do.
The claim: (a) <= (b) + (c), within the +-1 % one solve at a time varies by (profiles/r04_ab_noise_and_emit_under_overlap.txt).
    python tools/candidates_time.py [B]        output: profiles/candidates_time.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('igt-mpc-int_amd', 'oracle', 'tests', ''):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch  # noqa: E402

from bench import HBM_PEAK_GBS  # noqa: E402
from candidate_cases import per_scenario_candidates  # noqa: E402
from helpers import host_params  # noqa: E402
from igtmpc import BatchSolver  # noqa: E402
from igtmpc.cinf import cinf_halfplanes  # noqa: E402
from igtmpc.scenarios import make_batch  # noqa: E402

WARMUP, STEPS, N = 5, 20, 20
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(STEPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.asarray(ms)


b = make_batch(B, N=N, dtype=np.float64)
dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
       for a in (b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'])]
for C in (256, 64):
    U_host = per_scenario_candidates(b['u_prev'], host_params(N=N), C, N)
    U = torch.from_numpy(U_host).cuda()
    with BatchSolver(N=N, C=C, dtype='f64', cand_mode='table') as s:
        s.set_cinf(*cinf_halfplanes())
        s.set_candidate_table(U_host[0])
        out_a = s.solve_candidates(*dev[:4], U, obs_xy=dev[4])
        out_b = s.solve(*dev)
        torch.cuda.synchronize()
        solved = int((out_a['status'] == 0).sum()), int((out_b['status'] == 0).sum())
        ta = timed(lambda: s.solve_candidates(*dev[:4], U, obs_xy=dev[4], out=out_a))
        U0 = U[0:1].expand(B, -1, -1, -1).contiguous()
        out_d = s.solve_candidates(*dev[:4], U0, obs_xy=dev[4])
        torch.cuda.synchronize()
        same = all(torch.equal(out_d[k].nan_to_num(), out_b[k].nan_to_num()) for k in out_b)
        td = timed(lambda: s.solve_candidates(*dev[:4], U0, obs_xy=dev[4], out=out_d))
        del U0
        tb = timed(lambda: s.solve(*dev, out=out_b))
        s.set_profiling(True)
        s.solve_candidates(*dev[:4], U, obs_xy=dev[4], out=out_a)
        torch.cuda.synchronize()
        ka = s.kernel_ms()
        s.solve(*dev, out=out_b)
        torch.cuda.synchronize()
        kb = s.kernel_ms()
    floor = U.numel() * 8 / (HBM_PEAK_GBS * 1e9) * 1e3
    a, bb, d = float(np.median(ta)), float(np.median(tb)), float(np.median(td))
    print(f'B={B} C={C} N={N}: U is {U.numel() * 8 / 1e6:.1f} MB; solved {solved[0]} (a) / {solved[1]} (b) of {B}')
    print(f'  (a) solve_candidates         {a:8.4f} ms  (min {ta.min():.4f}, max {ta.max():.4f})   search {ka[0]:.4f}  emit {ka[1]:.4f}')
    print(f'  (b) solve, shared table U[0] {bb:8.4f} ms  (min {tb.min():.4f}, max {tb.max():.4f})   search {kb[0]:.4f}  emit {kb[1]:.4f}')
    print(f'  (c) streaming floor          {floor:8.4f} ms  ({HBM_PEAK_GBS:.0f} GB/s)')
    print(f'  (a)/(b) = {a / bb:.3f};  (a) - (b) - (c) = {a - bb - floor:+.4f} ms = {(a - bb - floor) / bb * 100:+.1f} % of (b): '
          f'the claim (a) <= (b) + (c) + 1 % is {"met" if a <= (bb + floor) * 1.01 else "NOT met"}', flush=True)
    print(f'  (d) solve_candidates, U[0] for every scenario {d:8.4f} ms  (min {td.min():.4f}, max {td.max():.4f}); answers equal to (b)\'s: {same};  '
          f'(d)/(b) = {d / bb:.3f}, (d) - (b) - (c) = {d - bb - floor:+.4f} ms', flush=True)
    del U
