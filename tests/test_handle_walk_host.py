"""The stations and walks of tests/handle_walk_cases.py against the plans the library would choose for them on 256 compute units.
tests/handle_walk_plan.cpp calls plan_search64, plan_candidates64 and plan_search32 from csrc/igt_launch.h itself (host side only,
address and undefined-behaviour sanitizers, a program of its own) and prints every field; nothing about the plans is restated
here.  Asserted: each station is on the side of the boundary it was chosen for, the stations reach every shipped search and emit
kernel of both precisions and both values of every decision about who initialises a piece of the workspace, every walk has every
ordered pair of its stations as consecutive calls, and the inputs of a station depend on (B, concurrency) alone.  No GPU."""
import pytest

import handle_walk_cases as HW


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    exe = HW.build_plan_program(tmp_path_factory.mktemp('handle_walk_plan'))
    if exe is None:
        pytest.skip('no hipcc')
    return HW.plans(exe, HW.N_CU_REFERENCE)


def test_what_the_plan_program_restates_is_what_the_library_does():
    """handle_walk_plan.cpp fills the plans' inputs as csrc/igt_api.hip does behind the handle -- the three lines its header lists.
    They are held to the source here, so that a change of solve_impl's or make_kp's rule fails this test and not silently the plans."""
    import os
    src = open(os.path.join(HW.CSRC, 'igt_api.hip')).read()
    assert 'const int waves_per_simd = h->concurrency >= 3 ? 1 : 2;' in src
    assert 'k.G = p.cand_mode == IGT_CAND_TABLE ? 1 : isqrt_exact(p.C);' in src
    assert 'k.hi_order = (k.h * vhi * (0.7 / p.l_r + 0.25) > 0.12) ? 1 : 0;' in src
    h, vhi, l_r = 0.1 / 4, 5.0 + 2.0, 4.47 / 2          # igt_params_default: dt / n_rk4, max(|v_min|, |v_max|) + 2, l_r
    assert not h * vhi * (0.7 / l_r + 0.25) > 0.12
    cpp = open(os.path.join(HW.ROOT, 'tests', 'handle_walk_plan.cpp')).read()
    assert cpp.count('// restated: ') == 3


def test_every_station_is_on_its_side_of_its_boundary(plans):
    for h, s, field, value in HW.EXPECTED:
        assert plans[h, s][field] == value, (h, s, field, plans[h, s])
    assert HW.plans_missed(plans) == []


def test_the_stations_reach_every_shipped_kernel_and_every_initialisation_rule(plans):
    """handle_walk_cases.REACHED, the one list of what must be reached: every shipped search and emit kernel of both precisions
    (WAVES3, ORACLE, LITERAL and UNITS_WAVES3 are the developer library's) and both values of every field that decides who
    initialises a piece."""
    by = lambda dtype, field: {p[field] for p in plans.values() if p['dtype'] == dtype}
    for field, values, dtype in HW.REACHED:
        assert by(dtype, field) == values, (dtype, field)
    assert {v != '0' for v in by('f32', 'ckpt_doubles')} == {False, True}
    # the value-network cost resets the compact list's length in both precisions and the keys in float
    assert by('f64', 'reset_rec_count') == {'0', '1'} and by('f32', 'reset_best_key') == {'0', '1'}


@pytest.mark.parametrize('name', list(HW.HANDLES))
def test_every_ordered_pair_of_stations_is_consecutive_in_the_walk(name):
    h = HW.HANDLES[name]
    k = len(h['stations'])
    walk = HW.walk_of(h)
    assert set(walk) == set(range(k))
    assert all(a != b for a, b in zip(walk, walk[1:]))
    if h['walk'] is None:
        assert len(walk) == k * (k - 1) + 1 and walk[0] == walk[-1]
    assert HW.consecutive_pairs(walk) == {(a, b) for a in range(k) for b in range(k) if a != b}
    # the shorter trail of the poisoned walks: every station, entered from another station, never twice from the same one
    short = HW.walk_of(h, short=True)
    assert set(short) == set(range(k)) and all(a != b for a, b in zip(short, short[1:]))
    assert len(HW.consecutive_pairs(short)) == len(short) - 1


@pytest.mark.parametrize('name', list(HW.HANDLES))
def test_stations_that_share_a_batch_size_and_concurrency_share_their_inputs(name):
    h = HW.HANDLES[name]
    ids = [s['id'] for s in h['stations']]
    assert len(set(ids)) == len(ids)
    seen = {}
    for s in h['stations']:
        key = (s['B'], s['conc'])      # the scenarios; a warm start on top of them is the station's own (its id says so)
        assert seen.setdefault(key, s['seed']) == s['seed'], (name, key)
        assert s['id'].endswith('-ws') == bool(s.get('ws'))
    assert max(s['B'] for s in h['stations']) <= 8200
