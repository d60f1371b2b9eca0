"""Non-finite and huge inputs of the solves: the poison table, its placement in a batch and the cases (tests only, no GPU).

A poison kind is (array, field, value): one element of one input array of one scenario is overwritten.  Arrays and fields:
    x0       x y s ey epsi v psi
    u_prev   a df
    kparams  b0 b1 Kv
    obs_xy   k0.x k0.y k1.x k1.y kN.x kN.y        obstacle 0 at node 0, 1, N (node 0 is not read by the device)
    u_ws     a df, on a scenario whose IGT_FLAG_WARM is set ('u_ws+') or clear ('u_ws-': the row is ignored)
    tv_sv    s v       enc  ego tv                 value-network cost only
Values: nan, +inf, -inf and a huge finite +-1e200 (float64, below the device's 1e300 guard) / +-3e38 (float32).  The float32 arrays
are poisoned after the cast, so the oracle (fed the device's arrays, up-cast exactly) sees what the device sees.

Placement (placement()): fixed, not drawn.  Scenario 0; scenario B - 1 (in a ragged last wave wherever 64 does not divide B); a
pair of adjacent scenarios; two inside one block of 64 consecutive scenarios (one emit wave); two inside one block of 64 / G (one
wave of the acceleration-row pass); every other poisoned scenario at least 3 from the next.  At most a quarter of a batch and at
most 60 scenarios, each with ONE kind.  A case takes every kind that only it can carry (u_ws, tv_sv, enc) and fills up from the
kinds every case can carry, starting where the case before it of the same dtype stopped, so the kinds rotate over the cases and
each appears in a float64 and in a float32 case (tests/test_nonfinite_cases_host.py).

What the oracle says about a kind decides how the device is held to it (tests/test_gpu_nonfinite.py):
    inert        obs_xy k0.*, u_ws-: the poisoned scenario's answer is the clean one, bit for bit;
    out of domain x0.psi / x0.epsi of +-huge: far outside the angles the solve is accurate for (include/igtmpc.h) -- isolation
                 and the signature only: the device may answer status 1 where the oracle solves;
    every other  parity with the oracle on the poisoned scenarios."""
import functools

import numpy as np

X0_FIELDS = ('x', 'y', 's', 'ey', 'epsi', 'v', 'psi')
VALUES = ('nan', '+huge', '+inf', '-huge', '-inf')
HUGE = {'f64': 1e200, 'f32': 3e38}
OBS_FIELDS = ('k0.x', 'k0.y', 'k1.x', 'k1.y', 'kN.x', 'kN.y')
# the kinds every case can carry, value-major: any window of the rotation mixes arrays and fields
BASE_FIELDS = [('x0', f) for f in X0_FIELDS] + [('u_prev', f) for f in ('a', 'df')] + [('kparams', f) for f in ('b0', 'b1', 'Kv')] + \
              [('obs_xy', f) for f in OBS_FIELDS]
BASE_KINDS = [(a, f, v) for v in VALUES for a, f in BASE_FIELDS]
WS_KINDS = [(a, f, v) for v in VALUES for a in ('u_ws+', 'u_ws-') for f in ('a', 'df')]
NET_KINDS = [(a, f, v) for v in VALUES for a, fs in (('tv_sv', ('s', 'v')), ('enc', ('ego', 'tv'))) for f in fs]
ALL_KINDS = BASE_KINDS + WS_KINDS + NET_KINDS
MAX_POISONED = 60
SEED = 2031


def value_of(name, dtype):
    if not isinstance(name, str):
        return name
    return {'nan': np.nan, '+inf': np.inf, '-inf': -np.inf, '+huge': HUGE[dtype], '-huge': -HUGE[dtype]}[name]


def is_inert(kind):
    return (kind[0] == 'obs_xy' and kind[1].startswith('k0.')) or kind[0] == 'u_ws-'


ANGLE_DOMAIN = 1.0e6      # include/igtmpc.h: |psi_0|, |epsi_0| up to here are rolled at full accuracy


def is_out_of_domain(kind):
    if kind[0] not in ('x0', 'x0|abs') or kind[1] not in ('psi', 'epsi'):
        return False
    return kind[2].endswith('huge') if isinstance(kind[2], str) else abs(kind[2]) > ANGLE_DOMAIN


# Headings outside (-pi, pi] (make_batch draws psi_0 from the four road directions only): multiples of pi / 2 where the
# Cody-Waite reduction of csrc/igt_math64.h sincos_reduced changes quadrant, 200 pi + 0.3 (|psi| = 630: ulp 1.1e-13, the oracle's
# own error in x, y about N v dt ulp = 1e-11), heading errors either side of QUADRANT0 = 0.78 -- and, as out-of-domain kinds,
# finite angles far beyond what the reduction is written for.  'x0|abs': the negative heading with IGT_FLAG_ABS_HEADING set.
_PSI = [np.pi, 1.5 * np.pi, 2 * np.pi, 7.5 * np.pi, 200 * np.pi + 0.3]
HEADING_KINDS = [('x0', 'psi', sgn * v) for v in _PSI for sgn in (1.0, -1.0)] + [('x0|abs', 'psi', -v) for v in _PSI] + \
                [('x0', 'epsi', v) for v in (0.78, -0.78, 0.79, -0.79)]
FAR_ANGLE_KINDS = [('x0', f, sgn * v) for f in ('psi', 'epsi') for v in (1e10, 1e300) for sgn in (1.0, -1.0)]


def placement(B, G=16):
    """-> sorted indices of the poisoned scenarios of a batch of B (at most B / 4 and MAX_POISONED), by the rules of the module
    docstring."""
    per = 64 // G
    n = min(MAX_POISONED, B // 4)
    assert B >= 2 * per and n >= 4, (B, n)
    if B < 192:      # one emit wave or two: the adjacent pair is the pair of the row wave's block and of the emit wave's
        special = [0, per + 1, per + 2, B - 1]
    else:
        special = [0, 2 * per, 2 * per + 3, 40, 41, 69, 104, B - 1]
    out = list(special)
    stride = max(3, -(-(B - 108) // max(n - len(special), 1)))
    for p in range(108 + stride, B - 3, stride):
        if len(out) >= n:
            break
        out.append(p)
    return sorted(out)


def check_placement(idx, B, G=16):
    """The rules, asserted (the host test calls it for every case)."""
    idx = np.asarray(idx)
    per = 64 // G
    assert len(set(idx.tolist())) == len(idx) and (np.diff(idx) > 0).all()
    assert idx[0] == 0 and idx[-1] == B - 1
    assert len(idx) <= B // 4 and len(idx) <= MAX_POISONED
    gaps = np.diff(idx)
    assert (gaps == 1).sum() == 1, 'one pair of adjacent scenarios'
    assert np.bincount(idx // 64).max() >= 2, 'two in one emit wave'
    assert np.bincount(idx // per).max() >= 2, 'two in one wave of the row pass'
    # every other gap is at least 3, except inside the one row-wave block that is poisoned twice (gap 3 there anyway at G = 16)
    assert (gaps[gaps != 1] >= 3).all(), gaps


# ----------------------------------------------------------------------------- the cases
# name: (dtype, B, family, options).  Options: C, N, refine, net (the shipped checkpoint's scenario), ws (warm starts on two
# thirds of the batch, and the u_ws kinds), dev (IGT_DEV_FLAGS), conc (set_concurrency), polish (polish_iters), vpolish
# (set_value_polish on the device driver).  The order fixes the rotation of the kinds.
DEV_SEPARATE_QUEUES = 33554432      # igtmpc._lib
CASES = {
    'f64-capture-lattice': ('f64', 256, 'lattice', {}),
    'f64-capture-track': ('f64', 256, 'track', {}),
    'f64-capture-ramp_hold': ('f64', 256, 'ramp_hold', dict(ws=True)),
    'f64-capture-ramp_hold-refined': ('f64', 256, 'ramp_hold', dict(refine=1)),
    'f64-rows-lattice': ('f64', 1100, 'lattice', {}),
    'f64-rows-track': ('f64', 1100, 'track', dict(ws=True)),
    'f64-rows-lattice-separate-queues': ('f64', 1100, 'lattice', dict(dev=DEV_SEPARATE_QUEUES)),
    'f64-unsorted-track': ('f64', 6200, 'track', {}),
    'f64-pool-pieces': ('f64', 8200, 'lattice', {}),
    'f64-pool-overlap': ('f64', 4100, 'lattice', dict(conc=4)),
    'f64-pool-overlap-c64': ('f64', 4100, 'lattice', dict(conc=4, C=64, N=8)),
    'f64-net-lattice': ('f64', 300, 'lattice', dict(net=3)),
    'f64-net-ramp_hold-refined': ('f64', 300, 'ramp_hold', dict(net=3, refine=1)),
    'f64-polish-track': ('f64', 256, 'track', dict(polish=2)),
    'f64-value-polish': ('f64', 256, 'lattice', dict(net=3, vpolish=1)),
    'f64-headings-pool': ('f64', 8200, 'lattice', dict(headings=True)),
    'f64-headings-units': ('f64', 1100, 'lattice', dict(headings=True)),
    'f32-ckpt-track': ('f32', 600, 'track', dict(ws=True, rot=66)),      # rot: a window with 20 kinds that fail a family steering by feedback
    'f32-ckpt-lattice': ('f32', 600, 'lattice', {}),
    'f32-plain-lattice': ('f32', 2100, 'lattice', {}),
    'f32-net-lattice': ('f32', 300, 'lattice', dict(net=3)),
}
DEFAULTS = dict(C=256, N=20, refine=0, net=0, ws=False, dev=0, conc=1, polish=0, vpolish=0, headings=False, rot=0)
POISON_CASES = [n for n, c in CASES.items() if not c[3].get('headings')]


def spec(name):
    dtype, B, cand, opt = CASES[name]
    return dict(DEFAULTS, name=name, dtype=dtype, B=B, cand=cand, **opt)


@functools.lru_cache(maxsize=None)
def case_kinds(name):
    """-> tuple of the case's kinds, one per poisoned scenario, in the order of placement()'s indices."""
    s = spec(name)
    if s['headings']:
        return tuple(HEADING_KINDS + FAR_ANGLE_KINDS)
    n = n_poisoned(s)
    start = 0
    for other in CASES:                      # where the cases before it of the same dtype stopped in the base rotation
        if other == name:
            break
        o = spec(other)
        if o['dtype'] == s['dtype'] and not o['headings']:
            start += n_poisoned(o) - len(_own_kinds(o))
    start += s['rot']
    own = _own_kinds(s)
    base = [BASE_KINDS[(start + i) % len(BASE_KINDS)] for i in range(n - len(own))]
    # interleaved, so that the special places (scenario 0, the pairs) are not all taken by one array
    kinds = []
    while own or base:
        if base:
            kinds.append(base.pop(0))
        if own:
            kinds.append(own.pop(0))
    return tuple(kinds[:n])


def n_poisoned(s):
    return len(placement(s['B'], int(round(np.sqrt(s['C'])))))


def _own_kinds(s):
    return (list(WS_KINDS) if s['ws'] else []) + (list(NET_KINDS) if s['net'] else [])


def net_of(sc):
    """The shipped checkpoint with non-identity statistics, as tests/test_gpu_value_gradient.py _net."""
    from igtmpc import shipped_value_net
    rng = np.random.default_rng(100 + sc)
    return dict(shipped_value_net(sc), Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)),
                mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6), sigma_t=1.7, mu_t=-0.4)


def apply(args, kinds, idx, dtype, N):
    """A clean batch `args` (dict x0, u_prev, kparams, flags, obs, u_ws, tv_sv, enc in the device's dtype) with kinds[i] written
    into scenario idx[i] -> the poisoned copy.  The clean batch must carry IGT_FLAG_WARM where a 'u_ws+' kind goes and not
    where a 'u_ws-' kind goes (clean_and_poisoned sees to it)."""
    bad = {k: (None if v is None else v.copy()) for k, v in args.items()}
    for (arr, field, vname), b in zip(kinds, idx):
        v = value_of(vname, dtype)
        if arr in ('x0', 'x0|abs'):
            bad['x0'][b, X0_FIELDS.index(field)] = v
            if arr == 'x0|abs':
                bad['flags'][b] |= np.uint32(1)
        elif arr == 'u_prev':
            bad['u_prev'][b, ('a', 'df').index(field)] = v
        elif arr == 'kparams':
            bad['kparams'][b, ('b0', 'b1', 'Kv').index(field)] = v
        elif arr == 'obs_xy':
            k = {'k0': 0, 'k1': 1, 'kN': N}[field[:2]]
            bad['obs'][b, 0, ('x', 'y').index(field[3:]), k] = v
        elif arr in ('u_ws+', 'u_ws-'):
            assert bool(args['flags'][b] & 2) == (arr == 'u_ws+'), (arr, b)
            bad['u_ws'][b, ('a', 'df').index(field), N // 2] = v
        elif arr == 'tv_sv':
            bad['tv_sv'][b, ('s', 'v').index(field)] = v
        elif arr == 'enc':
            bad['enc'][b, ('ego', 'tv').index(field)] = v
        else:
            raise KeyError(arr)
    return bad


@functools.lru_cache(maxsize=4)
def clean_and_poisoned(name):
    """-> (spec, clean args, poisoned args, idx, kinds).  The clean batch is make_batch(B, N, seed = SEED); ramp-hold and tracking
    cases with ws carry parity_cases.warm_args' warm starts on two thirds of it, the flag then set or cleared where a u_ws kind
    needs it -- in the clean batch, which the poisoned one copies."""
    from igtmpc.scenarios import make_batch
    import parity_cases as PC
    s = spec(name)
    npdt = np.float64 if s['dtype'] == 'f64' else np.float32
    G = int(round(np.sqrt(s['C'])))
    kinds = case_kinds(name)
    idx = placement(s['B'], G)
    if s['headings']:      # every second place, the first and the last scenario among them
        idx = (idx[:-1:2] + idx[-1:])[-len(kinds):]
    assert len(idx) == len(kinds), (name, len(idx), len(kinds))
    b = make_batch(s['B'], N=s['N'], dtype=npdt, seed=SEED)
    args = dict(x0=b['x0'], u_prev=b['u_prev'], kparams=b['kparams'], flags=b['flags'].copy(), obs=b['obs_xy'], u_ws=None,
                tv_sv=b['tv_sv'], enc=b['enc'])
    if s['ws']:
        args['u_prev'], args['u_ws'], args['flags'] = PC.warm_args(b, npdt, s['N'])
        args['flags'] = args['flags'].copy()
        for (arr, _, _), i in zip(kinds, idx):
            if arr == 'u_ws+':
                args['flags'][i] |= np.uint32(2)
            elif arr == 'u_ws-':
                args['flags'][i] &= ~np.uint32(2)
    bad = apply(args, kinds, idx, s['dtype'], s['N'])
    return s, args, bad, np.asarray(idx), kinds


def compared_positions(name):
    """Positions, among the case's poisoned scenarios, of those the oracle is asked about: all but the out-of-domain kinds."""
    return np.asarray([i for i, k in enumerate(case_kinds(name)) if not is_out_of_domain(k)])


def parity_case(name):
    """The poisoned scenarios the oracle is asked about as a parity_cases case: what the oracle runs on and
    tools/parity_floors.py measures."""
    import parity_cases as PC
    s, _, bad, idx, _ = clean_and_poisoned(name)
    idx = idx[compared_positions(name)]
    sub = {k: (None if v is None else np.ascontiguousarray(v[idx])) for k, v in bad.items()}
    dtype, cand, net = s['dtype'], s['cand'], (net_of(s['net']) if s['net'] else None)
    f32 = dtype == 'f32'
    # DESIGN.md section 6, as the seeded draws of parity_cases.fuzz_case take them: 1e-9 in float64; float32: 1e-5 with the
    # threshold / break-point / near-tie set-asides of its family and cost
    tol, utol = (PC.REL_TOL, 1e-7 if cand != 'track' else PC.REL_TOL) if f32 else (1e-9, 1e-12 if cand == 'track' else 1e-7)
    eps, tie = ((2e-5, 2e-5) if net or cand == 'track' else (PC.F32_EPS, PC.F32_TIE)) if f32 else (1e-9, 1e-9)
    return PC.make_case(f'nonfinite[{name}]', dtype, sub, N=s['N'], C=s['C'], cand=cand, refine=s['refine'], net=net,
                        cinf=PC.cinf_default(), eps=eps, tie=tie, tol=tol, utol=utol, ctol=2e-5 if f32 and net else None,
                        use_bp=f32, need=5)


def nonfinite_rows(passes):
    """[n] bool: scenarios the oracle answers status 1 BECAUSE of a non-finite state or cost: in its last pass every candidate
    carries verdict bit 6 or a non-finite cost, so no threshold is near."""
    r = passes[-1]
    finite = ((r['mask'] & 64) == 0) & np.isfinite(r['J'])
    return (r['status'] == 1) & ~finite.any(axis=1)
