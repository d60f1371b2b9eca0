"""Long-lived handles (tests/test_gpu_handle_walk.py, tests/test_handle_walk_host.py): the stations, the walks and the helpers
the two files share.  Data and helpers only -- no fixtures, no test.

Every entry that needs scratch carves it from the handle's one workspace (csrc/igt_api.hip carve_work), which grows and is never
cleared; where a piece lands and who writes it first depends on the batch size and on the plan (csrc/igt_launch.h
plan_search64, plan_candidates64, plan_search32; DESIGN.md section 4 has the table).  A STATION is one call with fixed inputs:
(entry, B, set_concurrency value, seed of the inputs).  Its reference answer is the same call on a fresh handle.  A WALK is an
order of calls on one handle in which every ordered pair of distinct stations is consecutive at least once (a closed Euler trail
of the complete digraph on the stations: k (k - 1) calls), so every station runs on what every other one left behind.

Shapes: C = 256, N = 20, n_rk4 = 4, one obstacle, default limits; at 256 compute units the batch sizes are the smallest on each
side of every boundary of the plans (EXPECTED below names the station that reaches each plan value there;
tests/handle_walk_plan.cpp prints the plans from the header itself).

Inputs depend on (handle, B, concurrency) alone, so two stations of a handle that share both -- the table handle's solve,
roll-out and per-scenario solve at B = 64 -- read the same scenarios; a warm-start station adds u_ws and the flag bit to them."""
import contextlib
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

import np_oracle as O
from candidate_cases import per_scenario_candidates
from helpers import host_params
from igtmpc._lib import DEV_KEEP_QUEUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')
N_CU_REFERENCE = 256          # the compute units the batch sizes were chosen for (MI355X)
SOLVE_KEYS = ('x', 'u', 'cost', 'argmin', 'status')
RESULT_KEYS = dict(solve=SOLVE_KEYS, solve_candidates=SOLVE_KEYS, rollout_all=('X', 'U', 'cost', 'viol'),
                   rollout_candidates=('X', 'U', 'cost', 'viol'), cost_gradient=('cost', 'grad'), terminal_value=('V', 'dV'))
SOLVE_ENTRIES = ('solve', 'solve_candidates')
DEVICE_ENTRIES = ('solve', 'solve_candidates', 'cost_gradient', 'terminal_value')      # the others take host arrays only


def st(entry, B, conc=1, **extra):
    """A station.  extra: ws (a warm start u_ws with flags & 2), vp (set_value_polish(vp) under the device driver around the call)."""
    sid = f'{entry}-{B}-c{conc}' + ('-ws' if extra.get('ws') else '') + (f'-vp{extra["vp"]}' if extra.get('vp') else '')
    return dict(id=sid, entry=entry, B=B, conc=conc, seed=3000 + 13 * B + conc, **extra)


def _handle(name, dtype, cand, stations, cost='progress', N=20, dev=0, walk=None, **solver_kw):
    return dict(name=name, dtype=dtype, cand=cand, cost=cost, N=N, C=256, dev=dev, stations=stations, walk=walk, solver_kw=solver_kw)


_VN_STATIONS = [st('solve', 33), st('solve', 300), st('solve', 1100), st('rollout_all', 64), st('cost_gradient', 200),
                st('terminal_value', 1000), st('solve', 256, vp=1)]
_TABLE_STATIONS = [st('solve', 64), st('solve', 300), st('rollout_all', 64), st('cost_gradient', 200), st('solve_candidates', 64),
                   st('rollout_candidates', 32)]
HANDLES = {h['name']: h for h in (
    _handle('f64-lattice', 'f64', 'lattice', [st('solve', 33), st('solve', 300), st('solve', 1100), st('solve', 6200),
                                              st('solve', 8200), st('solve', 4096, 3), st('solve', 300, 3)]),
    # capture on the queues (DEV_KEEP_QUEUES) next to the units: the walk is given, 33 -> 300 -> 33
    _handle('f64-lattice-keep-queues', 'f64', 'lattice', [st('solve', 33), st('solve', 300)], dev=DEV_KEEP_QUEUES, walk=(0, 1, 0)),
    # B = 1100 with and without a warm start under one plan and on the same scenarios (u_ws and flags & 2 are the whole difference);
    # the station at concurrency 3 is another batch
    _handle('f64-track', 'f64', 'track', [st('solve', 33), st('solve', 300), st('solve', 1100), st('solve', 1100, ws=True),
                                          st('solve', 300, 3), st('solve', 6200)]),
    _handle('f64-ramp-hold', 'f64', 'ramp_hold', [st('solve', 33), st('solve', 300), st('solve', 1100)], refine_iters=2),
    _handle('f64-lattice-value', 'f64', 'lattice', _VN_STATIONS, cost='value_net', value_polish_driver='device'),
    _handle('f64-table', 'f64', 'table', _TABLE_STATIONS, polish_iters=1),
    _handle('f64-table-n40', 'f64', 'table', _TABLE_STATIONS, N=40, polish_iters=1),      # the candidate search's direct kernel
    _handle('f32-lattice', 'f32', 'lattice', [st('solve', 300), st('solve', 2048), st('solve', 2049), st('solve', 6200),
                                              st('solve', 4096, 3)]),
    _handle('f32-track', 'f32', 'track', [st('solve', 300), st('solve', 2049), st('solve', 6200)]),
    _handle('f32-lattice-value', 'f32', 'lattice', [st('solve', 33), st('solve', 300), st('solve', 2049)], cost='value_net'),
)}

# The plan values the stations are there for, and the station that reaches each at N_CU_REFERENCE compute units:
# (handle, station, field of the plan line, value).  test_handle_walk_host.py asserts every line at 256 compute units; the GPU test
# asserts them on such a device and skips, naming the stations, on another.
EXPECTED = [
    ('f64-lattice', 'solve-33-c1', 'search_kernel', 'CAPTURE_STATIC'), ('f64-lattice', 'solve-33-c1', 'emit_kernel', 'GATHER'),
    ('f64-lattice-keep-queues', 'solve-33-c1', 'search_kernel', 'CAPTURE_QUEUES'),
    ('f64-lattice', 'solve-300-c1', 'search_kernel', 'UNITS'), ('f64-lattice', 'solve-300-c1', 'separate_queue_builder', '1'),
    ('f64-lattice', 'solve-300-c1', 'emit_kernel', 'PIECES'), ('f64-lattice', 'solve-300-c1', 'live_rows', '0'),
    ('f64-lattice', 'solve-1100-c1', 'live_rows', '1'), ('f64-lattice', 'solve-1100-c1', 'rows_build_queues', '1'),
    ('f64-lattice', 'solve-1100-c1', 'rows_threads', '256'), ('f64-lattice', 'solve-1100-c1', 'memset_counters', '0'),
    ('f64-lattice', 'solve-6200-c1', 'live_rows', '1'), ('f64-lattice', 'solve-6200-c1', 'rows_build_queues', '0'),
    ('f64-lattice', 'solve-6200-c1', 'separate_queue_builder', '0'), ('f64-lattice', 'solve-6200-c1', 'memset_counters', '1'),
    ('f64-lattice', 'solve-6200-c1', 'search_kernel', 'UNITS'),
    ('f64-lattice', 'solve-8200-c1', 'search_kernel', 'POOL'), ('f64-lattice', 'solve-8200-c1', 'memset_counters', '1'),
    ('f64-lattice', 'solve-8200-c1', 'emit_priority', '0'),
    ('f64-lattice', 'solve-4096-c3', 'search_kernel', 'POOL'), ('f64-lattice', 'solve-4096-c3', 'rows_build_queues', '1'),
    ('f64-lattice', 'solve-4096-c3', 'rows_threads', '64'), ('f64-lattice', 'solve-4096-c3', 'emit_kernel', 'ONE_PIECE'),
    ('f64-lattice', 'solve-4096-c3', 'emit_priority', '3'),
    ('f64-lattice', 'solve-300-c3', 'search_kernel', 'UNITS'), ('f64-lattice', 'solve-300-c3', 'emit_kernel', 'ONE_PIECE'),
    ('f64-table', 'solve_candidates-64-c1', 'search_kernel', 'CANDIDATES_STAGED'),
    ('f64-table-n40', 'solve_candidates-64-c1', 'search_kernel', 'CANDIDATES_DIRECT'),
    ('f32-lattice', 'solve-300-c1', 'ck_parts', '4'), ('f32-lattice', 'solve-300-c1', 'builds_queues', '1'),
    ('f32-lattice', 'solve-2048-c1', 'search_kernel', 'CHECKPOINTS'), ('f32-lattice', 'solve-2048-c1', 'emit_kernel', 'PIECES'),
    ('f32-lattice', 'solve-2049-c1', 'search_kernel', 'UNITS'), ('f32-lattice', 'solve-2049-c1', 'emit_kernel', 'ONE_PIECE'),
    ('f32-lattice', 'solve-2049-c1', 'ckpt_doubles', '0'),
    ('f32-lattice', 'solve-6200-c1', 'builds_queues', '0'), ('f32-lattice', 'solve-6200-c1', 'memset_counters', '1'),
    ('f32-track', 'solve-2049-c1', 'search_kernel', 'TRACK'), ('f32-track', 'solve-2049-c1', 'incumbents', '1'),
    ('f32-lattice', 'solve-2049-c1', 'incumbents', '0'), ('f32-lattice', 'solve-2049-c1', 'memset_counters', '0'),
]

# every value the stations must reach between them, by plan field: (field, values, precision of the plan)
REACHED = [
    ('search_kernel', {'CAPTURE_STATIC', 'CAPTURE_QUEUES', 'POOL', 'UNITS', 'CANDIDATES_STAGED', 'CANDIDATES_DIRECT'}, 'f64'),
    ('emit_kernel', {'GATHER', 'PIECES', 'ONE_PIECE'}, 'f64'),
    ('search_kernel', {'CHECKPOINTS', 'TRACK', 'UNITS'}, 'f32'),      # (WAVES3 is the developer library's)
    ('emit_kernel', {'PIECES', 'ONE_PIECE'}, 'f32'),
    ('memset_counters', {'0', '1'}, 'f64'), ('memset_counters', {'0', '1'}, 'f32'),
    ('live_rows', {'0', '1'}, 'f64'), ('rows_build_queues', {'0', '1'}, 'f64'), ('separate_queue_builder', {'0', '1'}, 'f64'),
    ('builds_queues', {'0', '1'}, 'f32'), ('incumbents', {'0', '1'}, 'f32'),
    ('rows_threads', {'64', '256'}, 'f64'), ('emit_priority', {'0', '3'}, 'f64'),
]


# ---------------------------------------------------------------------------------------------------------------- the walks
def euler_trail(k):
    """A closed trail through every arc of the complete digraph on k vertices, from vertex 0: k (k - 1) + 1 vertices (Hierholzer,
    arcs taken in ascending order: the same trail every time)."""
    if k == 1:
        return [0]
    nxt = {v: [w for w in range(k) if w != v][::-1] for v in range(k)}      # popped from the end: ascending
    stack, trail = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            trail.append(stack.pop())
    return trail[::-1]


def short_trail(k):
    """Every vertex at least once, each visit entered from another vertex and no vertex twice from the same one: 0 .. k-1 and
    back to 0 (2 k - 1 vertices; every vertex but the two ends is entered from both neighbours)."""
    return list(range(k)) + list(range(k - 2, -1, -1))


def walk_of(handle, short=False):
    """The station indices of the handle's walk."""
    if handle['walk'] is not None:
        return list(handle['walk'])
    k = len(handle['stations'])
    return short_trail(k) if short else euler_trail(k)


def consecutive_pairs(walk):
    return {(a, b) for a, b in zip(walk, walk[1:])}


# ------------------------------------------------------------------------------------------------------------- the plan lines
def plan_item(handle, station):
    """The station's argument of tests/handle_walk_plan.cpp, or None for an entry that runs no search."""
    if station['entry'] not in SOLVE_ENTRIES:
        return None
    return ','.join(str(v) for v in (handle['dtype'], handle['cand'], handle['cost'], handle['N'], handle['C'], station['B'],
                                     station['conc'], handle['dev'], int(station['entry'] == 'solve_candidates')))


def hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def build_plan_program(tmp_path):
    """tests/handle_walk_plan.cpp, host side only, under the address and undefined-behaviour sanitizers, as a program of its own
    (as tests/test_search_plan_host.py builds search_plan.cpp); -> its path, or None without hipcc."""
    cc = hipcc()
    if not cc:
        return None
    exe = tmp_path / 'handle_walk_plan'
    r = subprocess.run([cc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror',
                        '-Wno-unused-function', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                        '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'handle_walk_plan.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plans(exe, n_cu):
    """-> {(handle name, station id): dict(field -> value as printed)} for every station that runs a search."""
    keys, items = [], []
    for h in HANDLES.values():
        for s in h['stations']:
            item = plan_item(h, s)
            if item:
                keys.append((h['name'], s['id']))
                items.append(item)
    r = subprocess.run([exe, str(n_cu)] + items, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split('\n')
    assert len(lines) == len(items), r.stdout
    out = {}
    for key, item, line in zip(keys, items, lines):
        head, _, rest = line.partition(': ')
        assert head == item, (head, item)
        out[key] = dict(kv.split('=') for kv in rest.split())
        out[key]['dtype'] = item.split(',')[0]
    return out


def plans_missed(P):
    """What the stations do not reach on the device the plans P were printed for: -> list of messages, each naming a station
    (EXPECTED) or a plan value no station has (REACHED)."""
    missed = [f'{h}/{s}: {field} is {P[h, s][field]}, not {value}' for h, s, field, value in EXPECTED if P[h, s][field] != value]
    for field, values, dtype in REACHED:
        got = {p[field] for p in P.values() if p['dtype'] == dtype and field in p}
        if not values <= got:
            missed.append(f'{dtype} {field}: no station reaches {sorted(values - got)}')
    got = {p['ckpt_doubles'] != '0' for p in P.values() if p['dtype'] == 'f32'}
    if got != {False, True}:
        missed.append('f32 ckpt_doubles: zero and non-zero are not both reached')
    return missed


# ------------------------------------------------------------------------------------------------------------------ the inputs
def value_net():
    """V_GT_sc3 with the non-identity statistics of tests/test_gpu_value_gradient.py: nonfinite_cases.net_of, the recipe's one copy
    among the shared case modules."""
    from nonfinite_cases import net_of
    return net_of(3)


@functools.lru_cache(maxsize=None)
def shared_table(N):
    """The table handles' shared table: scenario 0's lattice (seed 1), and with it scenario 0's previous controls for every
    scenario of a table station (a table's controls are held to the rate limits from u_prev; parity_cases.leaf_case does the same)."""
    from igtmpc.scenarios import make_batch
    b = make_batch(1, N=N, dtype=np.float64, seed=1)
    U = np.ascontiguousarray(O.candidates_lattice(b['u_prev'][:1], host_params(N=N), 256)[0])
    U.setflags(write=False)
    return U, b['u_prev'][0].copy()


_INPUTS = {}


def inputs(handle, station):
    """The station's arrays in the handle's precision, built once and read-only: x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, and
    by entry u_ws (warm start), U (cost_gradient: [B,2,N]; the candidate entries: [B,C,2,N]) and sv (terminal_value)."""
    key = (handle['name'], station['B'], station['conc'], bool(station.get('ws')))
    if key in _INPUTS:
        return _INPUTS[key]
    from igtmpc.scenarios import make_batch
    npdt = np.float64 if handle['dtype'] == 'f64' else np.float32
    B, N = station['B'], handle['N']
    b = make_batch(B, N=N, dtype=npdt, seed=station['seed'])
    a = {k: b[k] for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc')}
    rng = np.random.default_rng(station['seed'] + 1)
    P = host_params(N=N)
    if handle['cand'] == 'table':
        a['u_prev'] = np.ascontiguousarray(np.broadcast_to(shared_table(N)[1], (B, 2)).astype(npdt))
        # per-scenario candidates: ramps around u_prev, the rate limit and the input box broken by the last ones
        a['Ucand'] = per_scenario_candidates(a['u_prev'], P, handle['C'], N, seed=station['seed'] + 2)
    # one control sequence per scenario (cost_gradient; the warm start): a ramp of random slope from u_prev, inside the box
    k = np.arange(1, N + 1)
    U = np.empty((B, 2, N))
    U[:, 0] = np.clip(a['u_prev'][:, 0:1] + rng.uniform(-1, 1, (B, 1)) * P.dt * P.jerk * k, P.a_min, P.a_max)
    U[:, 1] = np.clip(a['u_prev'][:, 1:2] + rng.uniform(-1, 1, (B, 1)) * 0.3 * P.dt * P.steer_rate * k, -P.df_max, P.df_max)
    a['U'] = U
    if station.get('ws'):
        a['u_ws'] = np.ascontiguousarray(U.astype(npdt))
        a['flags'] = a['flags'] | np.uint32(2)
    a['sv'] = np.ascontiguousarray(np.stack([b['x0'][:, 2] + rng.uniform(0, 8, B), b['x0'][:, 5]], axis=-1).astype(np.float64))
    for v in a.values():
        v.setflags(write=False)
    _INPUTS[key] = a
    return a


# ------------------------------------------------------------------------------------------------------------------ the calls
def open_solver(igt, handle, monkeypatch, poison=None):
    """The handle's BatchSolver.  The library reads IGT_DEV_FLAGS and IGT_DEV_POISON once, at igt_create: both are set for the
    length of this call only (poison None: unset -- the reference handles and the history walks)."""
    with monkeypatch.context() as m:
        m.delenv('IGT_DEV_POISON', raising=False)
        m.delenv('IGT_DEV_FLAGS', raising=False)
        if handle['dev']:
            m.setenv('IGT_DEV_FLAGS', str(handle['dev']))
        if poison is not None:
            m.setenv('IGT_DEV_POISON', str(poison))
        s = igt.BatchSolver(N=handle['N'], C=handle['C'], dtype=handle['dtype'], cand_mode=handle['cand'], cost_mode=handle['cost'],
                            **handle['solver_kw'])
    try:
        from igtmpc.cinf import cinf_halfplanes
        s.set_cinf(*cinf_halfplanes())
        if handle['cost'] == 'value_net':
            net = value_net()
            s.set_value_net(net['layers'], net['Wn'], net['mu_f'], net['sigma_t'], net['mu_t'])
        if handle['cand'] == 'table':
            s.set_candidate_table(shared_table(handle['N'])[0])
    except BaseException:
        s.close()
        raise
    return s


def _device(a):
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()      # (a copy: the inputs are read-only)


def _filled(shape, dtype, fill):
    """A device tensor whose every byte is `fill`."""
    import torch
    t = torch.empty(shape, dtype=dtype, device='cuda')
    t.view(torch.uint8).fill_(fill)
    return t


def run(s, handle, station, fill=None):
    """The station's call on the solver s -> dict of numpy arrays (RESULT_KEYS of the entry).  fill None: host arrays, the
    library stages them.  fill = a byte: device tensors, with out= buffers whose every byte is `fill` before the call, for the
    entries that take them (DEVICE_ENTRIES; the roll-out entries are host-mode and run as they do without fill)."""
    import torch
    a, e, B, N, C = inputs(handle, station), station['entry'], station['B'], handle['N'], handle['C']
    dev = fill is not None and e in DEVICE_ENTRIES
    D = _device if dev else (lambda x: x)
    td = torch.float64 if handle['dtype'] == 'f64' else torch.float32
    value = handle['cost'] == 'value_net'
    kw = dict(obs_xy=D(a['obs_xy']))
    if value:
        kw.update(tv_sv=D(a['tv_sv']), enc=D(a['enc']))
    s.set_concurrency(station['conc'])
    if station.get('vp'):
        s.set_value_polish(station['vp'])
    try:
        if e in SOLVE_ENTRIES:
            out = None
            if dev:
                out = dict(x=_filled((B, 7, N + 1), td, fill), u=_filled((B, 2, N), td, fill), cost=_filled((B,), td, fill),
                           argmin=_filled((B,), torch.int32, fill), status=_filled((B,), torch.int32, fill))
            pos = [D(a[k]) for k in ('x0', 'u_prev', 'kparams', 'flags')]
            if e == 'solve':
                r = s.solve(*pos, out=out, u_ws=D(a.get('u_ws')), **kw)
            else:
                r = s.solve_candidates(*pos, D(a['Ucand']), out=out, **kw)
        elif e == 'rollout_all':
            r = s.rollout_all(a['x0'], a['u_prev'], a['kparams'], a['flags'], **kw)
        elif e == 'rollout_candidates':
            r = s.rollout_candidates(a['x0'], a['u_prev'], a['kparams'], a['flags'], a['Ucand'], **kw)
        elif e == 'cost_gradient':
            out = dict(cost=_filled((B,), torch.float64, fill), grad=_filled((B, 2, N), torch.float64, fill)) if dev else None
            vn = dict(tv_sv=D(a['tv_sv']), enc=D(a['enc'])) if value else {}
            r = s.cost_gradient(D(a['x0']), D(a['kparams']), D(a['flags']), D(a['U']), out=out, **vn)
        elif e == 'terminal_value':
            out = dict(V=_filled((B,), torch.float64, fill), dV=_filled((B, 2), torch.float64, fill)) if dev else None
            r = s.terminal_value(D(a['sv']), D(a['tv_sv'].astype(np.float64)), D(a['enc'].astype(np.float64)), out=out)
        else:
            raise ValueError(e)
        if dev:
            torch.cuda.synchronize()
            r = {k: v.cpu().numpy() for k, v in r.items()}
    finally:
        if station.get('vp'):
            s.set_value_polish(0)
    return {k: r[k] for k in RESULT_KEYS[e]}


@contextlib.contextmanager
def side_stream():
    """A stream of the test's own for a capture, created on the HIP runtime the process has loaded and destroyed at the end -- not
    one of torch.cuda.Stream()'s, which come from a pool that lives as long as the process (DESIGN.md section 6;
    tests/test_gpu_candidates.py _side_stream has the story)."""
    import torch
    path = next(line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line)
    hip = ctypes.CDLL(path)
    st = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(st), 1) == 0          # hipStreamNonBlocking
    try:
        yield torch.cuda.ExternalStream(st.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(st) == 0


def same_bits(a, b):
    """Equal element for element by bit pattern (NaNs included: the payloads too)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_difference(got, ref):
    """-> None, or (key, index of the first element whose bits differ)."""
    for k in ref:
        if not same_bits(got[k], ref[k]):
            if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype:
                return k, 'shape or dtype'
            w = got[k].dtype.itemsize
            ga = np.ascontiguousarray(got[k]).view(f'u{w}').ravel()
            ra = np.ascontiguousarray(ref[k]).view(f'u{w}').ravel()
            i = int(np.flatnonzero(ga != ra)[0])
            return k, np.unravel_index(i, got[k].shape), int((ga != ra).sum())
    return None
