"""-m gpu : non-finite and huge inputs on every solve path -- isolation, the failure signature and parity with the oracle.

DESIGN.md section 1 / INTEGRATION.md: a problem with no finite feasible candidate returns status 1, argmin -1, cost +inf and NaN
rows, and it must not disturb its neighbours in the batch (igtmpc/evaluate.py carries on after a failed solve).  The scenarios
of a batch share waves, work queues, LDS tables and global keys; here a non-finite scenario goes through each of them.  The
poison table, its fixed placement and the cases are tests/nonfinite_cases.py (checked without a GPU by
tests/test_nonfinite_cases_host.py); every case solves the clean batch make_batch(B, seed = 2031) and the poisoned one on the same
solver and asserts
  a. isolation: every unpoisoned scenario's x, u, cost, argmin, status are the clean solve's, bit for bit;
  b. the signature: status 1 <-> argmin -1, cost +inf, all-NaN x and u; status 0 <-> finite x, u, cost, argmin >= 0 -- on every
     row, poisoned ones included, whatever the oracle says about them;
  c. parity on the poisoned scenarios with np_oracle.solve_batch / solve_batch_refined of the case's family: status 1 wherever
     the oracle fails BECAUSE every candidate is non-finite (nothing set aside: no threshold is near), helpers.compare_solve at the
     project's bars elsewhere (1e-9 float64; 1e-5 with the float32 set-asides), floors from tests/golden/parity_floors.json.  The
     out-of-domain kinds (x0.psi / x0.epsi of +-huge and the far angles of the heading cases) are held to a and b only: the
     device may answer status 1 where the oracle solves (include/igtmpc.h states the domain);
  d. inert kinds (obs_xy at node 0, u_ws without IGT_FLAG_WARM): the poisoned scenario itself is the clean solve, bit for bit.
Before anything is compared: the clean solve solves at least half of the unpoisoned scenarios, the oracle reports at least 20
poisoned scenarios as status 1 and at least 5 as solved.

The cases are the smallest shapes that reach each path on 256 compute units (C = 256, N = 20 unless stated):
  f64-capture-{lattice,track,ramp_hold}      B = 256   search_f64_kernel_cap, emit_gather_f64_kernel (ramp-hold: with warm starts)
  f64-capture-ramp_hold-refined              B = 256   refine_iters = 1: a failed first pass keeps its parameters, neighbours' second pass stays
  f64-rows-{lattice,track}                   B = 1100  accel_rows_kernel with the queue builder inside, 64-candidate units, emit in
                                                       pieces (tracking: incumbent keys, unit-rank-major queues, warm starts)
  f64-rows-lattice-separate-queues           B = 1100  DEV_SEPARATE_QUEUES: build_queues_kernel with the masks
  f64-unsorted-track                         B = 6200  unsorted queues, the counters reset by a memset
  f64-pool-pieces                            B = 8200  rollout_pool, one solve at a time, emit in pieces
  f64-pool-overlap                           B = 4100  set_concurrency(4): rollout_pool, one-piece emit at raised priority
  f64-pool-overlap-c64                       B = 4100  the same at C = 64, N = 8
  f64-net-lattice                            B = 300   value-network cost (checkpoint 3, non-identity statistics), tv_sv / enc kinds
  f64-net-ramp_hold-refined                  B = 300   ... ramp-hold with refine_iters = 1
  f64-polish-track                           B = 256   polish_iters = 2: a scenario with nothing to polish beside a polished one
  f64-value-polish                           B = 256   set_value_polish(1) on the device driver (64 trial rows per scenario)
  f64-headings-{pool,units}                  B = 8200 / 1100  headings outside (-pi, pi] through the solves (see below)
  f32-ckpt-{lattice,track}                   B = 600   checkpointed emit (tracking: incumbents, warm starts)
  f32-plain-lattice                          B = 2100  plain emit
  f32-net-lattice                            B = 300   value network: compact list, atomicMin winner, MFMA columns
A part with fewer compute units does not take the pool at these sizes and runs the unit kernels on both sides; the case still
passes and says so (the convention of test_gpu_pool_loop.py).

The polish cases: the oracle has no polish, so c holds them to the oracle's status, and on solved scenarios to a cost no higher
than the oracle's (a polish step is accepted only if strictly cheaper); a, b and d are unchanged.

Roll-out of all candidates (both dtypes, B = 16, C = 64): every candidate's viol word equals the oracle's mask, bit 6
(IGT_VIOL_NONFINITE) being a non-finite state or cost; finite costs match at the dtype's bar, the others are non-finite on the
device too; unpoisoned scenarios are the clean call bit for bit.

What these tests found when they first ran, and what was done (csrc/ and oracle/np_oracle.py):
  * x0.psi = +-huge (and any finite angle far outside the reduction's domain): status 0 with NaN x, y rows wherever the search
    had skipped the Cartesian rows (obstacles out of reach), float64 and float32 -- the emit wave now refuses |psi_0|, |epsi_0|
    beyond 1e6 (inputs_refused) and the header states the domain;
  * a NaN in a warm start (and, by the same clamps, in u_prev): solved towards a box limit where the oracle has no finite
    candidate -- refused by the emit wave as well;
  * kparams with b0 = +inf / NaN / huge or b1 = -inf on a turning route: the device took K = 0 where pw_const gives -Kv behind
    b1; a non-finite Kv: K = 0 behind the arc where Kv - Kv is NaN, and in float32 0 * Kv = NaN before the arc -- the device
    side was the one that did not restate pw_const: load_scenario now restates any triple as an ordered arc with the same K,
    and the float path's arc share multiplies a finite factor where the share is 0;
  * non-finite tv_sv / enc: solved with the value of a saturated network (the clamped tanh hides a NaN; an infinite feature
    saturates it) -- both value-network paths now give such an entry a NaN cost, as igt_terminal_value_f64 already did;
  * a NaN obstacle coordinate: the oracle's np.max voided the WHOLE collision verdict, the device ignores that node alone -- the
    oracle's verdict reductions are NaN-ignoring now (np.fmax; bit-identical on NaN-free inputs).
Isolation (a) and the inert kinds (d) held on every path from the first run.

Headings: make_batch draws psi_0 from the four road directions, so nothing else rolls another heading through the library's own
Cody-Waite reduction (csrc/igt_math64.h sincos_reduced).  test_headings_outside_the_principal_range compares a float64 rollout_all
with the oracle at 1e-9 on every trajectory for psi_0 in {+-pi, +-3pi/2, +-2pi, +-7.5pi, +-(200pi + 0.3)} (IGT_FLAG_ABS_HEADING
on the negative ones as well) and epsi_0 in {+-0.78, +-0.79}, either side of QUADRANT0; the heading cases put the same values
through the pool and unit solves.  At |psi| = 630 ulp(psi) is 1.1e-13 and the oracle's own error in x, y about N v dt ulp = 1e-11:
the bar belongs to the device.  Angles near 1e6 are not compared (ulp 1.2e-10: the oracle, which evaluates sin(psi_k + beta) at every
step, is the less accurate side); finite angles far beyond (1e10, 1e300) are out-of-domain kinds: a and b.
"""
import numpy as np
import pytest

import nonfinite_cases as NF
import np_oracle as O
import parity_cases as PC
from helpers import REL_TOL, measure, oracle_params, rel_err

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _solve(s, a, net):
    pos = [a['x0'], a['u_prev'], a['kparams'], a['flags'], a['obs']] + ([a['tv_sv'], a['enc']] if net else [])
    o = s.solve(*pos, u_ws=a['u_ws'])
    return {k: np.array(o[k]) for k in KEYS}


def check_signature(got, label):
    st = got['status']
    assert ((st == 0) | (st == 1)).all(), label
    bad = st == 1
    assert (got['argmin'][bad] == -1).all() and np.isposinf(got['cost'][bad]).all(), (label, 'status 1 without argmin -1, cost +inf')
    assert np.isnan(got['x'][bad]).all() and np.isnan(got['u'][bad]).all(), (label, 'status 1 with a row that is not all NaN')
    ok = ~bad
    assert (got['argmin'][ok] >= 0).all() and np.isfinite(got['cost'][ok]).all(), (label, 'status 0 without a winner')
    rows = ok & ~(np.isfinite(got['x']).all(axis=(-1, -2)) & np.isfinite(got['u']).all(axis=(-1, -2)))
    assert not rows.any(), (label, 'status 0 with non-finite rows in scenarios', np.flatnonzero(rows)[:8].tolist())


def _says_which_search(s, spec):
    """The pool's batch bound (csrc/igt_launch.h plan_search64) restated for the message only."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    slots = n_cu * 4 * (1 if spec['conc'] >= 3 else 2)
    if spec['name'].startswith(('f64-pool', 'f64-headings-pool')):
        print(f"{spec['name']}: {n_cu} compute units, " + ('the pool search runs' if spec['B'] >= 4 * slots else
                                                           'fewer than four scenarios per wave slot: the 64-candidate units run on both sides'))


@pytest.mark.parametrize('name', list(NF.CASES))
def test_poisoned_scenarios_are_isolated_and_match_the_oracle(igt, monkeypatch, name):
    spec, clean_in, bad_in, idx, kinds = NF.clean_and_poisoned(name)
    case = NF.parity_case(name)
    pos = NF.compared_positions(name)
    oracle = PC.oracle_passes_quiet(case)
    ref = oracle[0][-1]
    nonfinite = NF.nonfinite_rows(oracle[0])
    print(f'{name}: {len(idx)} poisoned of {spec["B"]}, {len(pos)} asked of the oracle: status 1 in {(ref["status"] == 1).sum()} '
          f'({nonfinite.sum()} of them with every candidate non-finite), solved {(ref["status"] == 0).sum()}')
    if not spec['headings']:
        assert (ref['status'] == 1).sum() >= 20 and (ref['status'] == 0).sum() >= 5, name
    else:
        assert (ref['status'] == 0).sum() >= 5, name

    if spec['dev']:
        monkeypatch.setenv('IGT_DEV_FLAGS', str(spec['dev']))
    kw = {}
    if spec['polish']:
        kw['polish_iters'] = spec['polish']
    if spec['vpolish']:
        kw.update(value_polish_iters=spec['vpolish'], value_polish_driver='device')
    with PC.open_solver(igt, case, **kw) as s:
        if spec['conc'] != 1:
            s.set_concurrency(spec['conc'])
        _says_which_search(s, spec)
        clean = _solve(s, clean_in, spec['net'])
        got = _solve(s, bad_in, spec['net'])

    keep = np.ones(spec['B'], dtype=bool)
    keep[idx] = False
    assert (clean['status'][keep] == 0).mean() >= 0.5, (name, 'the clean solve solves too few scenarios', (clean['status'][keep] == 0).mean())
    # every assertion below is made, and all that failed are reported together: one run says everything about a case
    problems = []

    def attempt(check, *a):
        try:
            check(*a)
        except AssertionError as e:
            problems.append(str(e)[:2000])

    # ---- b. the signature, on every row of both solves
    attempt(check_signature, clean, name + ' (clean)')
    attempt(check_signature, got, name)
    for kind, b in zip(kinds, idx):
        if got['status'][b] == 0 and not (np.isfinite(got['x'][b]).all() and np.isfinite(got['u'][b]).all()):
            problems.append(f'status 0 with non-finite rows: scenario {b}, kind {kind}')
    # ---- a. isolation: no unpoisoned scenario is left out
    for k in KEYS:
        same = np.array([np.array_equal(got[k][b], clean[k][b], equal_nan=True) for b in np.flatnonzero(keep)])
        if not same.all():
            problems.append(f'isolation: {k} of unpoisoned scenarios moved: {np.flatnonzero(keep)[~same][:8].tolist()}')
    # ---- d. inert kinds
    for kind, b in zip(kinds, idx):
        if NF.is_inert(kind):
            for k in KEYS:
                if not np.array_equal(got[k][b], clean[k][b], equal_nan=True):
                    problems.append(f'inert kind {kind} moved {k} of scenario {b}')
    # ---- c. parity on the poisoned scenarios
    sub = {k: got[k][idx[pos]] for k in KEYS}
    for i in np.flatnonzero((sub['status'] != ref['status']) | (sub['argmin'] != ref['argmin'])):
        print(f'   differs from the oracle: scenario {idx[pos[i]]}, kind {kinds[pos[i]]}: device status {sub["status"][i]} argmin '
              f'{sub["argmin"][i]} cost {sub["cost"][i]:.12g}, oracle status {ref["status"][i]} argmin {ref["argmin"][i]} cost {ref["cost"][i]:.12g}')
    wrong = nonfinite & (sub['status'] != 1)
    if wrong.any():
        problems.append(f'solved although every candidate is non-finite: {[kinds[i] for i in pos[wrong]]}')
    if spec['polish'] or spec['vpolish']:
        m, amb, _ = measure(oracle[0], case['P'], oracle[1], oracle[2], case['eps'], case['tie'], case['use_bp'])
        differ = ~amb & (sub['status'] != ref['status'])
        if differ.any():
            problems.append(f'status differs from the oracle: {[kinds[i] for i in pos[differ]]}')
        sol = ~amb & (ref['status'] == 0) & (sub['status'] == 0)
        assert sol.sum() >= 5
        if not (sub['cost'][sol] <= ref['cost'][sol] + case['tol'] * np.maximum(1.0, np.abs(ref['cost'][sol]))).all():
            problems.append('a polished cost above the oracle\'s unpolished one')
    else:
        attempt(PC.check_case, case, sub, oracle)
    assert not problems, '\n'.join([name] + problems)


# ----------------------------------------------------------------------------- roll-out of all candidates
# the reduced list: a NaN state, an infinite speed (0 * inf in the terminal set's facets), a huge coordinate, a NaN obstacle node
ROLLOUT_KINDS = [('x0', 's', 'nan'), ('x0', 'v', '+inf'), ('x0', 'x', '+huge'), ('obs_xy', 'k1.x', 'nan')]


def _rollout_inputs(dtype, kinds):
    from igtmpc.scenarios import make_batch
    npdt = np.float64 if dtype == 'f64' else np.float32
    b = make_batch(16, dtype=npdt, seed=NF.SEED)
    a = dict(x0=b['x0'], u_prev=b['u_prev'], kparams=b['kparams'], flags=b['flags'], obs=b['obs_xy'], u_ws=None,
             tv_sv=b['tv_sv'], enc=b['enc'])
    idx = NF.placement(16, 8)
    NF.check_placement(idx, 16, 8)
    return a, NF.apply(a, kinds, idx, dtype, 20), np.asarray(idx)


def _oracle_all(a, P, cinf):
    f = lambda k: np.asarray(a[k], dtype=np.float64)
    with np.errstate(all='ignore'):
        r = O.solve_batch(f('x0'), f('u_prev'), f('kparams'), a['flags'], f('obs'), cinf[0], cinf[1], P, C=64, return_all=True)
    mask = r['mask'] | np.where(np.isfinite(r['J']), 0, 64)        # IGT_VIOL_NONFINITE: a non-finite state or cost
    return r, mask


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_rollout_all_of_poisoned_scenarios(igt, dtype):
    clean_in, bad_in, idx = _rollout_inputs(dtype, ROLLOUT_KINDS)
    cinf = PC.cinf_default()
    with igt.BatchSolver(dtype=dtype, C=64) as s:
        P = oracle_params(s)
        s.set_cinf(*cinf)
        roll = lambda a: s.rollout_all(a['x0'], a['u_prev'], a['kparams'], a['flags'], a['obs'])
        clean, got = roll(clean_in), roll(bad_in)
    keep = np.ones(16, dtype=bool)
    keep[idx] = False
    for k in ('X', 'U', 'cost', 'viol'):
        assert np.array_equal(got[k][keep], clean[k][keep], equal_nan=True), k
    ref, mask = _oracle_all(bad_in, P, cinf)
    assert (mask[idx] & 64).any() and (mask[idx] == 0).any()
    tol, eps = (1e-9, 1e-9) if dtype == 'f64' else (REL_TOL, 1e-6)      # (float32 verdicts: test_rollout_all_f32_within_1e5's width)
    with np.errstate(invalid='ignore'):
        clear = ~(np.abs(ref['g'] - P.feas_tol) <= eps)
    if dtype == 'f32':
        x0 = O.apply_flags(bad_in['x0'].astype(np.float64), bad_in['flags'])[:, None, :]
        with np.errstate(all='ignore'):
            bp = O.breakpoint_distance(x0, ref['U'], bad_in['kparams'].astype(np.float64)[:, None, :], P)
        clear &= ~(bp <= PC.F32_EPS)
    assert clear.mean() > 0.99
    differ = clear & (got['viol'] != mask)
    assert not differ.any(), (np.argwhere(differ)[:8].tolist(), got['viol'][differ][:8], mask[differ][:8])
    fin = np.isfinite(ref['J'])
    assert rel_err(got['cost'][fin & clear], ref['J'][fin & clear]).max() <= tol
    assert not np.isfinite(got['cost'][~fin]).any()


# ----------------------------------------------------------------------------- headings outside (-pi, pi]
def test_headings_outside_the_principal_range(igt):
    from igtmpc.scenarios import make_batch
    b = make_batch(16, dtype=np.float64, seed=NF.SEED)
    a = dict(x0=b['x0'], u_prev=b['u_prev'], kparams=b['kparams'], flags=b['flags'].copy(), obs=b['obs_xy'], u_ws=None,
             tv_sv=b['tv_sv'], enc=b['enc'])
    a['flags'][:] &= ~np.uint32(1)
    kinds = [k for k in NF.HEADING_KINDS if k[0] == 'x0'] + [k for k in NF.HEADING_KINDS if k[0] == 'x0|abs'][3:]
    assert len(kinds) == 16
    a = NF.apply(a, kinds, range(16), 'f64', 20)
    assert (a['flags'] & 1).sum() == 2
    cinf = PC.cinf_default()
    with igt.BatchSolver(dtype='f64') as s:
        P = oracle_params(s)
        s.set_cinf(*cinf)
        got = s.rollout_all(a['x0'], a['u_prev'], a['kparams'], a['flags'], a['obs'])
    ref = O.solve_batch(a['x0'], a['u_prev'], a['kparams'], a['flags'], a['obs'], cinf[0], cinf[1], P, return_all=True)
    assert np.isfinite(ref['X']).all()
    err = rel_err(got['X'], ref['X']).max(axis=(1, 2, 3))
    print('worst relative error per scenario:', ' '.join(f'{k[2]:+.4g}:{e:.1e}' for k, e in zip(kinds, err)))
    assert err.max() < 1e-9
    assert rel_err(got['U'], ref['U']).max() == 0.0
    assert rel_err(got['cost'], ref['J']).max() < 1e-9
    clear = np.abs(ref['g'] - P.feas_tol) > 1e-9
    assert (got['viol'][clear] == ref['mask'][clear]).all()
