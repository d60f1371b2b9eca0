"""No GPU: the host side of tests/test_gpu_nonfinite.py -- the poison table (tests/nonfinite_cases.py), its placement, and what
the oracle alone says about every case.

  * the placement rules hold in every case (scenario 0, scenario B - 1, one adjacent pair, two in one emit wave, two in one wave
    of the row pass, every other gap at least 3, at most a quarter of the batch);
  * every kind appears in a float64 and in a float32 case, and the u_ws kinds sit on scenarios with the flag they need;
  * the oracle reports at least 20 of a case's poisoned scenarios as status 1 and at least 5 as solved, and the clean batch's
    first 64 unpoisoned scenarios are solved by at least half (the GPU test asserts that of the whole clean device solve);
  * the inert kinds leave the oracle's answer as it is, bit for bit;
  * the recorded floors of the nonfinite[...] comparisons are held to the inputs by tests/test_parity_floors_host.py, which
    takes its keys from parity_cases.all_cases -- checked here: every case is among them."""
import numpy as np
import pytest

import nonfinite_cases as NF
import np_oracle as O
import parity_cases as PC


@pytest.mark.parametrize('name', NF.POISON_CASES)
def test_placement_rules(name):
    s = NF.spec(name)
    G = int(round(np.sqrt(s['C'])))
    idx = NF.placement(s['B'], G)
    NF.check_placement(idx, s['B'], G)
    assert len(NF.case_kinds(name)) == len(idx)
    if s['B'] % 64:
        assert idx[-1] // 64 == s['B'] // 64, 'scenario B - 1 sits in the ragged last wave'


def test_small_batch_placement():
    for G in (8, 16):
        NF.check_placement(NF.placement(16, G), 16, G)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_every_kind_is_covered(dtype):
    assert len(set(NF.ALL_KINDS)) == len(NF.ALL_KINDS) == 5 * (7 + 2 + 3 + 6 + 4 + 4)
    seen = set()
    for name in NF.POISON_CASES:
        if NF.spec(name)['dtype'] == dtype:
            seen |= set(NF.case_kinds(name))
    assert set(NF.ALL_KINDS) <= seen, sorted(set(NF.ALL_KINDS) - seen)


@pytest.mark.parametrize('name', list(NF.CASES))
def test_poison_is_what_the_table_says(name):
    """The poisoned batch differs from the clean one in exactly the poisoned scenarios, one element each (and the flag of an
    'x0|abs' kind); float32 arrays hold the float32 value."""
    s, clean, bad, idx, kinds = NF.clean_and_poisoned(name)
    npdt = np.float64 if s['dtype'] == 'f64' else np.float32
    changed = np.zeros(s['B'], dtype=int)
    for k in clean:
        if clean[k] is None:
            assert bad[k] is None
            continue
        assert bad[k].dtype == clean[k].dtype and (k == 'flags' or clean[k].dtype == npdt)
        d = ~((bad[k] == clean[k]) | (np.isnan(bad[k].astype(np.float64)) & np.isnan(clean[k].astype(np.float64))))
        if k != 'flags':
            changed += d.reshape(s['B'], -1).sum(axis=1)
        else:
            assert set(np.flatnonzero(d).tolist()) <= {int(b) for kd, b in zip(kinds, idx) if kd[0] == 'x0|abs'}
    assert (changed[idx] <= 1).all() and changed.sum() == changed[idx].sum()
    for kd, b in zip(kinds, idx):      # a straight route carries b0 = b1 = +inf already: the one poison that can change nothing
        assert changed[b] == 1 or (kd[0] == 'kparams' and kd[2] == '+inf' and clean['kparams'][b, 2] == 0), (kd, int(b))
    for kd, b in zip(kinds, idx):
        if kd[0] in ('u_ws+', 'u_ws-'):
            assert bool(clean['flags'][b] & 2) == (kd[0] == 'u_ws+')


@pytest.mark.parametrize('name', list(NF.CASES))
def test_oracle_side_conditions(name):
    s, clean, bad, idx, kinds = NF.clean_and_poisoned(name)
    case = NF.parity_case(name)
    pos = NF.compared_positions(name)
    passes, _, _ = PC.oracle_passes_quiet(case)
    ref = passes[-1]
    n1, n0 = int((ref['status'] == 1).sum()), int((ref['status'] == 0).sum())
    print(f'{name}: status 1 in {n1} (every candidate non-finite: {NF.nonfinite_rows(passes).sum()}), solved {n0}')
    assert n0 >= 5
    if not s['headings']:
        assert n1 >= 20
    # the same scenarios, clean: the inert kinds' answers are the clean ones bit for bit, and the clean batch is mostly solved
    keep = np.setdiff1d(np.arange(s['B']), idx)[:64]
    rows = np.concatenate([idx[pos], keep])
    sub = {k: (None if v is None else np.ascontiguousarray(v[rows])) for k, v in clean.items()}
    cp = PC.oracle_passes_quiet(dict(case, args=sub, B=len(rows)))[0][-1]
    assert (cp['status'][len(pos):] == 0).mean() >= 0.5
    for i, p in enumerate(pos):
        if NF.is_inert(kinds[p]):
            for k in ('x', 'u', 'cost', 'argmin', 'status'):
                assert np.array_equal(ref[k][i], cp[k][i], equal_nan=True), (kinds[p], k)


def test_cases_are_registered_for_the_floors():
    keys = {k for k, _ in PC.all_cases()}
    assert {f'nonfinite[{n}]' for n in NF.CASES} <= keys
