"""-m gpu : with three or more solves in flight (igt_set_concurrency) the persistent float64 search leaves a reserve of wave slots
to the other lanes' emit and row passes (igt_launch.h search64_grid): it launches fewer waves, each of which dequeues more items.
Which wave rolls which scenario changes, what a scenario's roll-out computes does not, so a solve must be the same bits -- x, u,
cost, argmin, status -- alone with the device to itself (concurrency 1: every slot, two waves per SIMD), with concurrency 4 and
the reserve, and with concurrency 4 and the reserve switched off (DEV_NO_RESERVE); and so must every lane of four handles that
solve side by side on four streams.  f64, C = 256, N = 8; the lattice at B = 4096, the smallest batch at which the pool kernel
runs with igt_set_concurrency(4) on 256 compute units.  (The 64-candidate unit kernels take no reserve: no tracking case.)
"""
import numpy as np
import pytest

from igtmpc._lib import DEV_NO_RESERVE

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')
N, C, B = 8, 256, 4096
IN = ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy')


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _cinf():
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes()


def _batch(seed):
    from igtmpc.scenarios import make_batch
    return make_batch(B, N=N, dtype=np.float64, seed=seed)


def _solver(igt, conc):
    s = igt.BatchSolver(dtype='f64', cand_mode='lattice', N=N, C=C, n_obs=1)
    s.set_cinf(*_cinf())
    s.set_concurrency(conc)
    return s


def _solve(igt, monkeypatch, b, flags, conc):
    monkeypatch.setenv('IGT_DEV_FLAGS', str(flags))
    with _solver(igt, conc) as s:
        o = s.solve(*[b[k] for k in IN])
    monkeypatch.delenv('IGT_DEV_FLAGS')
    return {k: np.asarray(o[k]) for k in KEYS}


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.fixture(scope='module')
def alone(igt):
    """seed -> the batch and its solve with the device to itself (concurrency 1), computed once per seed"""
    mp = pytest.MonkeyPatch()
    cache = {}

    def get(seed):
        if seed not in cache:
            b = _batch(seed)
            cache[seed] = (b, _solve(igt, mp, b, 0, 1))
        return cache[seed]
    yield get
    mp.undo()


def test_reserve_on_and_off_equal_the_solve_alone(igt, monkeypatch, alone):
    b, ref = alone(2027)
    assert (ref['status'] == 0).mean() > 0.2, 'too few feasible scenarios to compare winners'
    on = _solve(igt, monkeypatch, b, 0, 4)
    off = _solve(igt, monkeypatch, b, DEV_NO_RESERVE, 4)
    _same(on, ref, 'concurrency 4, reserve on')
    _same(off, ref, 'concurrency 4, reserve off')
    _same(on, off, 'reserve on against off')


def test_four_lanes_with_the_reserve_equal_the_solve_alone(igt, alone):
    import torch
    F = 4
    sets = [alone(2027 + q) for q in range(F)]
    dev = [[torch.from_numpy(h[k].view(np.int32) if h[k].dtype == np.uint32 else h[k]).cuda() for k in IN] for h, _ in sets]
    solvers = [_solver(igt, F) for _ in range(F)]
    try:
        for q in range(F):                   # the workspaces grow on first use: not while overlapped
            solvers[q].solve(*dev[q])
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(F)]
        for rnd in range(3):
            outs = [None] * F
            for q in range(F):
                with torch.cuda.stream(streams[q]):
                    outs[q] = solvers[q].solve(*dev[q])
            torch.cuda.synchronize()
            for q in range(F):
                _same({k: outs[q][k].cpu().numpy() for k in KEYS}, sets[q][1], ('in flight', rnd, q))
    finally:
        for s in solvers:
            s.close()
