#!/usr/bin/env python3
"""What the polish of the winner (igtmpc.h polish_iters) buys and what it costs, on the device.  Needs the GPU and scipy.

    python tools/polish_gap.py gap  [n_scenarios=256] [processes=16]     # gap to the NLP optimum
    python tools/polish_gap.py time [--parent-lib PATH] [--repeats 5]     # milliseconds per solve, one solve at a time
    python tools/polish_gap.py loop [episodes=512]                        # closed loop with polish_iters 0 and 2
every mode takes  --grad fd|adjoint  (igtmpc.h igt_set_polish_gradient; default fd)  and  --step gradient|newton  (igt_set_polish_step;
default gradient; newton takes the analytic gradient whatever --grad says); time also  --N 20|40 ,  --B 4096,65536  and
--families lattice,ramp-hold,tracking

gap : the scenarios of tools/nlp_gap.py, solved by the device (float64) with the lattice, ramp-hold and tracking families x
      polish_iters 0, 1, 2, 4; gap = J - J_opt, J_opt the SLSQP optimum of oracle/nlp_quality.py started from the best answer
      any of them found (one optimum per scenario).
time: HIP events around solve(), B = 4096 and 65 536, N = 20, device tensors, one solve at a time after a warm-up; every
      configuration is a fresh child process, this library and --parent-lib (a build of the parent commit, same ABI) taking
      turns, `repeats` rounds; per configuration the median of each child's medians and the spread over the rounds.
      polish_iters 0 / 1 / 2 for the three families, refine_iters = 2 beside them for the tracking family.  With --grad adjoint
      the rows with polish_iters > 0 are measured in both gradient modes, side by side.  With --step newton only the rows with
      polish_iters 1 and 2 are measured: this library's adjoint and Newton modes and --parent-lib's adjoint mode, side by side.
loop: igtmpc.evaluate.run_closed_loop, tracking default, N = 20 and N = 40, 64 episodes for each of the 8 scenarios."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'igt-mpc-int_amd'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import numpy as np

FAMILIES = (('lattice', 'lattice'), ('ramp-hold', 'ramp_hold'), ('tracking', 'track'))


def _batch64(n, N=20):
    from igtmpc.scenarios import make_batch
    return {k: (np.asarray(v, dtype=np.float64) if v.dtype.kind == 'f' else v) for k, v in make_batch(n, N=N, dtype=np.float64).items()}


def _grad_kw(grad, step='gradient'):
    """BatchSolver keywords of the gradient mode and the step; none for the defaults, so that a library from before the setters
    still runs.  grad 'newton' (a row of the time table) is the Newton step."""
    if grad == 'newton':
        grad, step = 'adjoint', 'newton'
    if grad not in ('fd', 'adjoint'):
        sys.exit("--grad must be 'fd' or 'adjoint'")
    if step not in ('gradient', 'newton'):
        sys.exit("--step must be 'gradient' or 'newton'")
    return dict(**(dict(polish_grad=grad) if grad != 'fd' else {}), **(dict(polish_step=step) if step != 'gradient' else {}))


def _mode(grad, step):
    return 'newton' if step == 'newton' else grad


# ------------------------------------------------------------------------------------------------ gap
_G = {}


def _init(g):
    _G.update(g)


def _slsqp(job):
    import nlp_quality as Q
    i, u0 = job
    b, cinf, P = _G['b'], _G['cinf'], _G['P']
    r = Q.polish(b['x0'][i], b['u_prev'][i], b['kparams'][i], b['flags'][i], b['obs_xy'][i], cinf[0], cinf[1], P, u0, maxiter=100)
    return i, r['cost'], r['max_violation']


def gap(n=256, procs=16, grad='fd', step='gradient'):
    import multiprocessing as mp
    import igtmpc
    import np_oracle as O
    from igtmpc.cinf import cinf_halfplanes
    b, cinf, P = _batch64(n), cinf_halfplanes(), O.Params()
    _G.update(b=b, cinf=cinf, P=P)
    rows = {}
    for name, cand in FAMILIES:
        for k in (0, 1, 2, 4):
            with igtmpc.BatchSolver(dtype='f64', cand_mode=cand, polish_iters=k, **_grad_kw(grad, step)) as s:
                s.set_cinf(*cinf)
                rows[(name, k)] = s.solve(b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'])
    J = np.stack([np.where(r['status'] == 0, r['cost'], np.inf) for r in rows.values()])
    best = J.argmin(axis=0)
    sols = list(rows.values())
    jobs = [(i, sols[best[i]]['u'][i]) for i in range(n) if np.isfinite(J[:, i].min())]
    with mp.get_context('spawn').Pool(procs, initializer=_init, initargs=(dict(b=b, cinf=cinf, P=P),)) as pool:
        res = pool.map(_slsqp, jobs, chunksize=1)
    J_opt = np.full(n, np.nan)
    for i, c, viol in res:
        if viol < 1e-6:
            J_opt[i] = min(c, J[:, i].min())
    ok = np.isfinite(J_opt)
    print(f'{n} scenarios of the benchmark generator, device solves (float64), polish {_mode(grad, step)}; {len(jobs)} solved by at least one row; optimum '
          f'(SLSQP, violation < 1e-6) for {ok.sum()}, mean J_opt {J_opt[ok].mean():.4f}')
    for (name, k), Jf in zip(rows, J):
        m = ok & np.isfinite(Jf)
        g = Jf[m] - J_opt[m]
        J0 = J[list(rows).index((name, 0))]
        print(f'{name:10s} polish_iters {k}: solves {np.isfinite(Jf).mean() * 100:5.1f} %   gap mean {g.mean():.4f}  median {np.median(g):.4f}  '
              f'p90 {np.quantile(g, 0.9):.4f}  max {g.max():.4f}   mean cost drop {(J0[m] - Jf[m]).mean():.4f}   ({m.sum()} scenarios)')


# ------------------------------------------------------------------------------------------------ time
def _time_child(cand, B, polish, refine, grad='fd', N=20, solves=30, warm=10):
    """one configuration in this process: median milliseconds of `solves` solves, each timed by its own pair of events"""
    import torch
    import igtmpc
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.scenarios import make_batch
    b = make_batch(B, N=N, dtype=np.float64)
    dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).contiguous().cuda()
           for a in (b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'])]
    kw = dict(polish_iters=polish, **_grad_kw(grad)) if polish else {}
    with igtmpc.BatchSolver(dtype='f64', cand_mode=cand, N=N, refine_iters=refine, **kw) as s:
        s.set_cinf(*cinf_halfplanes())
        out = s.solve(*dev)
        for _ in range(warm):
            s.solve(*dev, out=out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(solves):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.solve(*dev, out=out)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    print(json.dumps(dict(ms=float(np.median(ms)), lo=float(np.min(ms)), hi=float(np.max(ms)))))


def time_(parent_lib=None, repeats=5, grad='fd', N=20, Bs=(4096, 65536), step='gradient', families=None):
    _grad_kw(grad, step)
    newton = step == 'newton'
    fams = [f for f in FAMILIES if families is None or f[0] in families]
    configs = []
    for B in Bs:
        for name, cand in fams:
            for k in ((1, 2) if newton else (0, 1, 2)):
                for gm in (('adjoint', 'newton') if newton else ('fd', 'adjoint') if (k and grad == 'adjoint') else ('fd',)):
                    configs.append((name, cand, B, k, 0, gm))
        if not newton:
            configs.append(('tracking', 'track', B, 0, 2, 'fd'))
    libs = [('this', None)] + ([('parent', parent_lib)] if parent_lib else [])
    got = {}
    for r in range(repeats):
        for name, cand, B, k, refine, gm in configs:
            for lib, path in libs:
                if lib == 'parent' and (gm != 'adjoint' if newton else (gm != 'fd' or (k and grad == 'fd'))):
                    continue           # --grad: the parent has no adjoint mode, its polished rows are asked for beside the
                                       # adjoint ones; --step newton: the parent's adjoint mode beside this library's two
                env = dict(os.environ)
                if path:
                    env['IGT_LIB_PATH'] = os.path.abspath(path)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), '_child', cand, str(B), str(k), str(refine), gm, str(N)],
                                   env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:          # a child that failed: nothing more is started on the device
                    sys.exit(f'{lib} {name} B={B} polish_iters={k} {gm}: exit {p.returncode}\n{p.stderr[-2000:]}')
                got.setdefault((B, name, k, refine, gm, lib), []).append(json.loads(p.stdout.strip().splitlines()[-1])['ms'])
                print(f'round {r + 1}: B = {B} {name} polish_iters {k} {gm} {lib}: {got[(B, name, k, refine, gm, lib)][-1]:.3f} ms',
                      file=sys.stderr, flush=True)      # progress: the table comes at the end
    print(f'milliseconds per solve (HIP events, one solve at a time, N = {N}, float64); median of {repeats} child processes '
          f'[min .. max of their medians], libraries taking turns')
    for (B, name, k, refine, gm, lib), v in got.items():
        what = (f'polish_iters {k} {gm}' if k else 'polish_iters 0') if not refine else f'refine_iters {refine}'
        print(f'B = {B:6d}  {name:10s} {what:23s} {lib:6s}: {np.median(v):8.3f}  [{min(v):.3f} .. {max(v):.3f}]', flush=True)


# ------------------------------------------------------------------------------------------------ loop
def loop(episodes=512, grad='fd', step='gradient'):
    """the protocol of DESIGN.md section 9's closed-loop table (tools/closed_loop_probe.py): episodes / 8 per scenario, 8 scenarios"""
    from igtmpc.evaluate import run_closed_loop
    for N in (20, 40):
        for k in (0, 2):
            inf, dl, fs, ms = [], [], [], []
            for sc in range(1, 9):
                r = run_closed_loop(sc=sc, num_samples=episodes // 8, N=N, polish_iters=k, **_grad_kw(grad, step))
                inf.append(r['infeasible_ratio'].mean()); dl.append(r['deadlock'].mean())
                fs.append(r['x_data'][:, 2::7, -1].mean()); ms.append(r['solve_ms'][5:].mean())
            print(f'closed loop, tracking default, N = {N}, {episodes // 8} episodes x 8 scenarios, polish_iters {k} ({_mode(grad, step)}): infeasible steps '
                  f'{np.mean(inf) * 100:.1f} %, deadlock flag {np.mean(dl) * 100:.1f} %, mean final s {np.mean(fs):.1f} m, '
                  f'{np.mean(ms):.3f} ms per step', flush=True)


if __name__ == '__main__':
    a = sys.argv[1:]
    opt = lambda name, default: a[a.index(name) + 1] if name in a else default
    grad = opt('--grad', 'fd')
    step = opt('--step', 'gradient')
    pos = []                                   # positional arguments: what is left of the options and their values
    i = 1
    while i < len(a):
        if a[i].startswith('--'):
            i += 2
        else:
            pos.append(a[i]); i += 1
    if a and a[0] == '_child':
        _time_child(a[1], int(a[2]), int(a[3]), int(a[4]), *(a[5:6]), *(int(x) for x in a[6:7]))
    elif a and a[0] == 'gap':
        gap(*(int(x) for x in pos[:2]), grad=grad, step=step)
    elif a and a[0] == 'time':
        time_(opt('--parent-lib', None), int(opt('--repeats', 5)), grad, int(opt('--N', 20)),
              tuple(int(x) for x in opt('--B', '4096,65536').split(',')), step,
              opt('--families', None) and opt('--families', None).split(','))
    elif a and a[0] == 'loop':
        loop(*(int(x) for x in pos[:1]), grad=grad, step=step)
    else:
        sys.exit(__doc__)
