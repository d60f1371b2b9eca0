"""-m gpu : a long-lived handle answers what a fresh one answers, whatever its workspace held.

Every entry carves its scratch from the handle's one workspace, which grows and is never cleared (csrc/igt_api.hip carve_work);
where a piece lands and who initialises it depends on the batch size and the plan (DESIGN.md section 4 has the table).  The
stations and walks are tests/handle_walk_cases.py's: one handle per family and cost is walked so that every station runs behind
every other one, and every call's full result is compared, bit for bit (NaN payloads included), with the same call on a fresh
handle.  No tolerances anywhere in this file.

  history      the walk on a handle as the library ships;
  poison       the same on handles created with IGT_DEV_POISON = 0, 255, 90: the whole workspace holds that byte before every
               call (0: fresh memory made deterministic; 255: -1 as an index, NaN as a double, "none" as a key; 90: a huge counter,
               a large finite double, an index out of range), on the shorter trail;
  outputs      device tensors and out= buffers pre-filled with 0x00 and with 0xA5: both give the reference, unsolved rows included;
  concurrency  set_concurrency is read per call: 1, 4, 1 around one batch;
  capture      a captured solve replayed between eager solves of other plans on the same handle, none of which grows the workspace;
  refusals     a refused call between two identical solves changes nothing.

The roll-out entries take host arrays only (BatchSolver.rollout_all / rollout_candidates); in the walks on device tensors they run
on host arrays, like in the others, and their staging is the library's."""
import numpy as np
import pytest

import handle_walk_cases as HW

pytestmark = pytest.mark.gpu

POISONS = (0, 255, 90)


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


@pytest.fixture(scope='module')
def references(igt):
    """(handle name, station id) -> the station's result on a fresh handle with an unpoisoned workspace; each computed once, on
    first use, and read-only."""
    cache = {}

    def get(handle, station):
        key = (handle['name'], station['id'])
        if key not in cache:
            mp = pytest.MonkeyPatch()
            try:
                with HW.open_solver(igt, handle, mp) as s:
                    r = HW.run(s, handle, station)
            finally:
                mp.undo()
            for v in r.values():
                v.setflags(write=False)
            if station['entry'] in HW.SOLVE_ENTRIES:      # solved and unsolved scenarios, so that status == 1 rows are compared too
                solved = int((r['status'] == 0).sum())
                assert 0 < solved < station['B'], (key, solved)
                assert set(np.unique(r['status'])) == {0, 1}, key
            cache[key] = r
        return cache[key]
    return get


def _walk_and_compare(igt, references, monkeypatch, handle, poison=None, short=False, fill=None):
    stations = handle['stations']
    with HW.open_solver(igt, handle, monkeypatch, poison=poison) as s:
        prev = None
        for n, i in enumerate(HW.walk_of(handle, short=short)):
            got = HW.run(s, handle, stations[i], fill=fill)
            bad = HW.first_difference(got, references(handle, stations[i]))
            assert bad is None, (f'{handle["name"]}: call {n}, station {stations[i]["id"]} behind '
                                 f'{"a fresh workspace" if prev is None else stations[prev]["id"]}, poison {poison}, fill {fill}: '
                                 f'(key, first differing element, how many differ) = {bad}')
            prev = i


def _fresh(igt, handle, station, monkeypatch):
    with HW.open_solver(igt, handle, monkeypatch) as s:
        return HW.run(s, handle, station)


def test_the_stations_reach_the_plans_they_were_chosen_for(igt, tmp_path):
    """tests/handle_walk_plan.cpp for this device's compute units.  On 256 of them every plan value named in
    handle_walk_cases.EXPECTED / REACHED is reached; on another device the stations that miss theirs are named in a skip."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    exe = HW.build_plan_program(tmp_path)
    assert exe is not None, 'no hipcc'
    missed = HW.plans_missed(HW.plans(exe, n_cu))
    if n_cu == HW.N_CU_REFERENCE:
        assert missed == []
    elif missed:
        pytest.skip(f'{n_cu} compute units, not {HW.N_CU_REFERENCE}: ' + '; '.join(missed))


@pytest.mark.parametrize('name', list(HW.HANDLES))
def test_history(igt, references, monkeypatch, name):
    _walk_and_compare(igt, references, monkeypatch, HW.HANDLES[name])


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('name', list(HW.HANDLES))
def test_poison(igt, references, monkeypatch, name, poison):
    _walk_and_compare(igt, references, monkeypatch, HW.HANDLES[name], poison=poison, short=True)


@pytest.mark.parametrize('name', list(HW.HANDLES))
def test_outputs_are_written_in_full(igt, references, monkeypatch, name):
    """Whatever the output buffers held -- zeros, 0xA5 bytes -- every element is the reference's afterwards (and so the two runs
    equal each other), unsolved rows included: x and u NaN, cost +inf, argmin -1 (include/igtmpc.h)."""
    for fill in (0x00, 0xA5):
        _walk_and_compare(igt, references, monkeypatch, HW.HANDLES[name], short=True, fill=fill)


@pytest.mark.parametrize('name,B', [('f64-lattice', 4096), ('f32-lattice', 2048)])
def test_concurrency_is_per_call(igt, monkeypatch, name, B):
    """igt_set_concurrency changes the plan of the next solve, not its answer: 1, then 4, then 1 around the same batch on one handle,
    all equal to each other and to the fresh handles' answers under either setting."""
    h = HW.HANDLES[name]
    at = {c: HW.st('solve', B, c) for c in (1, 4)}
    for c in at:      # the same scenarios under both settings
        at[c]['seed'] = at[1]['seed']
    fresh = {c: _fresh(igt, h, at[c], monkeypatch) for c in at}
    assert HW.first_difference(fresh[4], fresh[1]) is None
    assert 0 < (fresh[1]['status'] == 0).sum() < B
    with HW.open_solver(igt, h, monkeypatch) as s:
        for n, c in enumerate((1, 4, 1)):
            bad = HW.first_difference(HW.run(s, h, at[c]), fresh[1])
            assert bad is None, (name, n, c, bad)


@pytest.mark.parametrize('name,B', [('f64-lattice', 4096), ('f32-lattice', 2048)])
def test_a_captured_solve_next_to_other_plans(igt, monkeypatch, name, B):
    """The solve of B scenarios is captured on a stream of the test's own (a pool stream must not carry a
    capture) and replayed three times; between the replays the handle solves B = 33 and B = 300 eagerly -- other plans, other
    carvings of the same workspace -- and the graph's outputs are overwritten with 0xA5.  Every replay is the fresh handle's
    answer.

    The eager solves must not grow the workspace: growth frees the arena whose addresses the graph holds (include/igtmpc.h), and
    the largest arena is not the largest batch's -- in float64 B = 33 keeps 12.8 MB of trajectories where B = 4096 carves 4.1 MB.
    So every plan is warmed before the capture, and that none of them would grow the arena afterwards is asserted the one way the
    library shows it: each is captured once as well (never replayed), which ensure_work refuses with IGT_E_STATE if it had to
    grow."""
    import torch
    h = HW.HANDLES[name]
    big, others = HW.st('solve', B), [HW.st('solve', 33), HW.st('solve', 300)]
    ref, other_refs = _fresh(igt, h, big, monkeypatch), [_fresh(igt, h, o, monkeypatch) for o in others]
    assert 0 < (ref['status'] == 0).sum() < B
    keys = ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy')
    bufs = [HW._device(HW.inputs(h, big)[k]) for k in keys]
    other_bufs = [[HW._device(HW.inputs(h, o)[k]) for k in keys] for o in others]
    with HW.open_solver(igt, h, monkeypatch) as s:
        with HW.side_stream() as side:
            with torch.cuda.stream(side):             # every plan once, eagerly: the workspace takes its largest size here
                other_outs = [s.solve(*ob) for ob in other_bufs]
                out = s.solve(*bufs)
            side.synchronize()
            for ob, oo in zip(other_bufs, other_outs):      # no later eager solve grows the arena: its capture is not refused
                probe = torch.cuda.CUDAGraph()
                with torch.cuda.graph(probe, stream=side):
                    s.solve(*ob, out=oo)
                del probe
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):    # a single stream, no parallel branches
                s.solve(*bufs, out=out)
            for rnd in range(3):
                for t in out.values():
                    t.view(torch.uint8).fill_(0xA5)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                got = {k: out[k].cpu().numpy() for k in HW.SOLVE_KEYS}
                bad = HW.first_difference(got, ref)
                assert bad is None, (name, 'replay', rnd, bad)
                for o, o_ref in zip(others, other_refs):
                    bad = HW.first_difference(HW.run(s, h, o, fill=0xA5), o_ref)
                    assert bad is None, (name, 'eager', rnd, o['id'], bad)
            del g


def test_refusals_leave_no_trace(igt, references, monkeypatch):
    """A bad `mem`, a null buffer and set_value_polish under capture are refused before anything is enqueued: the solve behind
    them equals the solve before them."""
    import torch
    from igtmpc import _lib as L
    h = HW.HANDLES['f64-lattice-value']
    station = h['stations'][1]                        # solve, B = 300
    ref = references(h, station)
    a = HW.inputs(h, station)
    B, N = station['B'], h['N']
    with HW.open_solver(igt, h, monkeypatch) as s:
        assert HW.first_difference(HW.run(s, h, station), ref) is None
        out = dict(x=np.empty((B, 7, N + 1)), u=np.empty((B, 2, N)), cost=np.empty(B), argmin=np.empty(B, np.int32),
                   status=np.empty(B, np.int32))
        P = lambda v: v.ctypes.data
        ins = [P(a[k]) for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc')] + [None]
        outs = [P(out[k]) for k in HW.SOLVE_KEYS]
        E_INVALID = -1                                # include/igtmpc.h IGT_E_INVALID
        # a bad mem
        assert s._solve(s._h, B, *ins, *outs, 77, None) == E_INVALID
        # a null buffer: an input, then an output
        assert s._solve(s._h, B, None, *ins[1:], *outs, L.IGT_MEM_HOST, None) == E_INVALID
        assert s._solve(s._h, B, *ins, *outs[:-1], None, L.IGT_MEM_HOST, None) == E_INVALID
        # the value polish under capture
        bufs = [HW._device(a[k]) for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc')]
        with HW.side_stream() as side:
            with torch.cuda.stream(side):
                dout = s.solve(*bufs[:5], tv_sv=bufs[5], enc=bufs[6])
            side.synchronize()
            s.set_value_polish(1)
            g = torch.cuda.CUDAGraph()
            with pytest.raises(igt.IgtError, match='stream capture'):
                with torch.cuda.graph(g, stream=side):
                    s.solve(*bufs[:5], tv_sv=bufs[5], enc=bufs[6], out=dout)
            del g
        s.set_value_polish(0)
        torch.cuda.synchronize()
        bad = HW.first_difference(HW.run(s, h, station), ref)
        assert bad is None, bad
