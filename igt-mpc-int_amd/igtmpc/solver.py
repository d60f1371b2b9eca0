"""BatchSolver -- Python face of the C ABI (include/igtmpc.h).

One BatchSolver replaces, for a whole batch of (scenario, ego) problems, what the
reference does one problem at a time with MPC_Planner.update_initial_condition /
update_predictions / solve (mpc.py:241-294, 383-406).

Buffers may be numpy arrays (host mode: the library stages them through HBM and
synchronises) or torch tensors on the solver's GPU (device mode: pointers are
handed over as they are and the work is enqueued on the given / current stream)."""
import ctypes as ct

import numpy as np

from . import _lib as L

_DT = {'f32': np.float32, 'f64': np.float64}
VALUE_POLISH_TRIALS = 64
VALUE_POLISH_DRIVERS = ('host', 'device')


def _is_torch(x):
    return hasattr(x, 'data_ptr') and hasattr(x, 'is_cuda')


def check_value_polish(iters, dtype, cost_mode):
    """What BatchSolver(value_polish_iters=) / set_value_polish refuse, before any GPU call (the driver asks it too)."""
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= iters <= 4:
        raise ValueError('value_polish_iters must be an integer in [0, 4]')
    if iters > 0 and dtype != 'f64':
        raise ValueError("value_polish_iters > 0 needs dtype='f64'")
    if iters > 0 and cost_mode != 'value_net':
        raise ValueError("value_polish_iters > 0 needs cost_mode='value_net' (the progress cost has polish_iters)")


def check_value_polish_driver(driver):
    """The name of who drives the polish under the value-network cost: 'host' (numpy, _value_polish_host) or 'device' (igtmpc.h
    igt_set_value_polish).  Refused before any GPU call."""
    if driver not in VALUE_POLISH_DRIVERS:
        raise ValueError(f"value_polish_driver must be 'host' or 'device', not {driver!r}")


class BatchSolver:
    def __init__(self, N=20, dt=0.1, n_rk4=4, C=256, n_obs=1, device=0, dtype='f32',
                 cand_mode='lattice', cost_mode='progress', polish_grad='fd', polish_step='gradient',
                 value_polish_iters=0, value_polish_driver='host', **limits):
        self._h = None
        self.lib = L.load()          # the shipped library -- or libigtmpc_dev.so when IGT_DEV_FLAGS asks for developer kernels
        if dtype not in _DT:
            raise ValueError("dtype must be 'f32' or 'f64'")
        self.dtype = dtype
        self.np_dtype = _DT[dtype]
        p = L.igt_params()
        self._check(self.lib.igt_params_default(ct.byref(p)))
        p.N, p.dt, p.n_rk4, p.C, p.n_obs = N, dt, n_rk4, C, n_obs
        p.cand_mode = {'lattice': L.IGT_CAND_LATTICE, 'table': L.IGT_CAND_TABLE,
                       'ramp_hold': L.IGT_CAND_RAMP_HOLD, 'track': L.IGT_CAND_TRACK}[cand_mode]
        p.cost_mode = {'progress': L.IGT_COST_PROGRESS, 'value_net': L.IGT_COST_VALUE_NET}[cost_mode]
        for k, v in limits.items():
            if not hasattr(p, k):
                raise TypeError(f'unknown parameter {k!r}')
            setattr(p, k, v)
        # polish of the winner (igtmpc.h polish_iters): float64 and the progress cost only -- refused here, before any GPU call
        if not 0 <= p.polish_iters <= 4:
            raise ValueError('polish_iters must be in [0, 4]')
        if p.polish_iters > 0 and dtype != 'f64':
            raise ValueError("polish_iters > 0 needs dtype='f64' (a forward difference of 1e-4 on a float cost is noise)")
        if p.polish_iters > 0 and cost_mode != 'progress':
            raise ValueError("polish_iters > 0 needs cost_mode='progress' (the value-network cost is not polished)")
        # gradient of the polish (igtmpc.h igt_set_polish_gradient): 'fd' forward differences (the default), 'adjoint' analytic
        if polish_grad not in ('fd', 'adjoint'):
            raise ValueError("polish_grad must be 'fd' or 'adjoint'")
        self.polish_grad = polish_grad
        # step of the polish (igtmpc.h igt_set_polish_step): 'gradient' the trials along the scaled -gradient (the default), 'newton'
        # half of them along the Gauss-Newton (LQ) direction, which takes the analytic gradient whatever polish_grad says
        if polish_step not in ('gradient', 'newton'):
            raise ValueError("polish_step must be 'gradient' or 'newton'")
        self.polish_step = polish_step
        # polish of the winner under the value-network cost (set_value_polish below): an explicit keyword, not a field of
        # igt_params -- float64 and cost_mode='value_net' only, refused here, before any GPU call
        check_value_polish(value_polish_iters, dtype, cost_mode)
        self.value_polish_iters = int(value_polish_iters)
        # ... and who takes its steps: 'host' (the default) this class from numpy, 'device' the library inside the solve
        check_value_polish_driver(value_polish_driver)
        self.value_polish_driver = value_polish_driver
        self.params = p
        self.device = device
        self.cost_mode = cost_mode
        self._cinf_args = self._net_args = self._vp_table = None      # what value_polish's trial handle is set up from
        h = ct.c_void_p()
        self._check(self.lib.igt_create(ct.byref(p), device, ct.byref(h)))
        self._h = h
        self.N, self.C, self.n_obs = N, C, n_obs
        self._solve = getattr(self.lib, f'igt_solve_batch_ws_{dtype}')
        self._rollout = getattr(self.lib, f'igt_rollout_batch_ws_{dtype}')
        self._cart = getattr(self.lib, f'igt_cartesian_euler_{dtype}')
        self._fstep = getattr(self.lib, f'igt_frenet_step_{dtype}')
        self._fcast = getattr(self.lib, f'igt_forecast_batch_{dtype}')
        self._fscene = getattr(self.lib, f'igt_forecast_scene_{dtype}')
        self._routes_set = False
        self._headings_set = False      # igt_set_route_headings, set lazily by the pose forecasts
        self._n_routes = 0
        if polish_grad != 'fd':      # the default needs no call: a library from before the setter still serves it
            self._check(self.lib.igt_set_polish_gradient(self._h, L.IGT_GRAD_ADJOINT))
        if polish_step != 'gradient':      # likewise
            self._check(self.lib.igt_set_polish_step(self._h, L.IGT_POLISH_STEP_NEWTON))
        self._vp_field = 0      # the handle's igt_set_value_polish field: the iterations under 'device', 0 under 'host'
        self._set_value_polish(self.value_polish_iters, value_polish_driver)      # likewise: no call while the field stays 0

    def _check(self, rc):
        L.check(rc, self.lib)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        self._drop_vp_table()
        if self._h is not None:
            self.lib.igt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------------ tables
    def set_cinf(self, A, b):
        """C_inf half-planes A[F,2] (v,a) <= b[F]   (mpc.py:88-104, 177-180)."""
        A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
        if len(A) != len(b):
            raise ValueError('A and b disagree')
        self._check(self.lib.igt_set_cinf(self._h, A.ctypes.data, b.ctypes.data, len(b)))
        self._cinf_args = (A.copy(), b.copy())
        self._drop_vp_table()

    def set_candidate_table(self, U):
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.shape != (self.C, 2, self.N):
            raise ValueError(f'candidate table must be [{self.C},2,{self.N}]')
        self._check(self.lib.igt_set_candidate_table(self._h, U.ctypes.data))

    def set_value_net(self, layers, Wn=None, mu_f=None, sigma_t=1.0, mu_t=0.0):
        """Terminal value network of the gt_mpc cost (mpc.py:108-127, 367-369; model.py:14-51).
        layers = [(W[out,in], b[out]), ...] (3 or 4 Linear layers, 6 -> 128 -> ... -> 1);
        Wn[6,6], mu_f[6]: input whitening x -> Wn (x - mu_f); sigma_t, mu_t: target de-normalisation.
        The reference's statistics come from a dataset that is not shipped: identity by default."""
        Wn = np.eye(6) if Wn is None else np.asarray(Wn, dtype=np.float64)
        mu_f = np.zeros(6) if mu_f is None else np.asarray(mu_f, dtype=np.float64)
        dims = [int(np.asarray(layers[0][0]).shape[1])] + [int(np.asarray(W).shape[0]) for W, _ in layers]
        flat = np.concatenate([np.concatenate([np.asarray(W, np.float64).ravel(), np.asarray(b, np.float64).ravel()])
                               for W, b in layers])
        dims_a = np.asarray(dims, dtype=np.int32)
        Wn_c, mu_c = np.ascontiguousarray(Wn), np.ascontiguousarray(mu_f)
        self._check(self.lib.igt_set_value_net(self._h, len(layers), dims_a.ctypes.data, flat.ctypes.data,
                                           Wn_c.ctypes.data, mu_c.ctypes.data, float(sigma_t), float(mu_t)))
        self._net_args = (layers, Wn_c.copy(), mu_c.copy(), float(sigma_t), float(mu_t))
        self._drop_vp_table()

    def set_concurrency(self, solves_in_flight):
        """Solves the caller keeps in flight on the device at a time, on other handles / streams (igtmpc.h igt_set_concurrency):
        from 3 on, the persistent search kernels take one wave per SIMD instead of two so that two of them run side by side."""
        self._check(self.lib.igt_set_concurrency(self._h, int(solves_in_flight)))

    def set_profiling(self, on=True):
        self._check(self.lib.igt_set_profiling(self._h, int(on)))

    def kernel_ms(self):
        a, b = ct.c_float(), ct.c_float()
        self._check(self.lib.igt_get_kernel_ms(self._h, ct.byref(a), ct.byref(b)))
        return a.value, b.value

    def algorithmic_bytes_per_solve(self):
        r, w = ct.c_int64(), ct.c_int64()
        es = 4 if self.dtype == 'f32' else 8
        self._check(self.lib.igt_algorithmic_bytes_per_solve(self._h, es, ct.byref(r), ct.byref(w)))
        return r.value, w.value

    # ------------------------------------------------------------------ marshalling
    def _prep(self, arrs, shapes, dtypes):
        """-> (mode, ptrs, keepalive).  All numpy (host) or all torch-cuda (device)."""
        torch_mode = any(_is_torch(a) for a in arrs if a is not None)
        ptrs, keep = [], []
        for a, shp, dt in zip(arrs, shapes, dtypes):
            if a is None:
                ptrs.append(None)
                continue
            if torch_mode:
                import torch
                if not _is_torch(a) or not a.is_cuda:
                    raise TypeError('device mode needs every buffer to be a CUDA torch tensor')
                want = {np.float32: torch.float32, np.float64: torch.float64, np.uint32: torch.int32,
                        np.int32: torch.int32, np.int64: torch.int64}[dt]
                if a.dtype != want and not (dt is np.uint32 and a.dtype in (torch.int32, torch.uint32)):
                    raise TypeError(f'tensor dtype {a.dtype} does not match {dt.__name__}')
                if a.device.index != self.device:
                    raise ValueError('tensor is on another device')
                if not a.is_contiguous():
                    raise ValueError('device buffers must be contiguous')
                if tuple(a.shape) != tuple(shp):
                    raise ValueError(f'shape {tuple(a.shape)} != {tuple(shp)}')
                ptrs.append(a.data_ptr())
                keep.append(a)
            else:
                b = np.ascontiguousarray(a, dtype=dt)
                if b.shape != tuple(shp):
                    raise ValueError(f'shape {b.shape} != {tuple(shp)}')
                ptrs.append(b.ctypes.data)
                keep.append(b)
        return (L.IGT_MEM_DEVICE if torch_mode else L.IGT_MEM_HOST), ptrs, keep

    def _stream_ptr(self, stream, torch_mode):
        """hipStream_t for the C ABI.  Device mode: the given stream, else torch's current stream.  torch's default
        stream has handle 0, which the C ABI reads as "the handle's own non-blocking stream" -- the kernels would
        then be unordered with the torch ops that produce their inputs and consume their outputs.  So in device
        mode ANY resolved handle of 0 (implicit, `stream=torch.cuda.default_stream()`, `stream=0`) names the legacy
        default stream explicitly (hipStreamLegacy == (hipStream_t)1).  Host mode keeps NULL: the library stages
        and synchronises on its own stream."""
        if stream is not None:
            ptr = int(getattr(stream, 'cuda_stream', stream) or 0)
        elif torch_mode:
            import torch
            ptr = int(torch.cuda.current_stream(self.device).cuda_stream or 0)
        else:
            return None
        if torch_mode and ptr == 0:
            ptr = 1
        return ptr or None

    # ------------------------------------------------------------------ one path to the solve and roll-out entries
    def _solve_inputs(self, B, x0, u_prev, kparams, flags, obs, tv_sv, enc, eighth, obs_rows=2):
        """The eight (array, shape) pairs every solve and roll-out entry takes, in ABI order.  obs_rows: 2 (obs_xy) or 3 (obs_pose);
        eighth: u_ws[B,2,N] or the per-scenario candidates U[B,C,2,N] with its shape."""
        return [(x0, (B, 7)), (u_prev, (B, 2)), (kparams, (B, 3)), (flags, (B,)), (obs, (B, self.n_obs, obs_rows, self.N + 1)),
                (tv_sv, (B, 2)), (enc, (B, 2)), eighth]

    def _new_out(self, spec, like, skip=()):
        """The dict an entry answers with, from spec = ((name, shape, dtype), ...): torch tensors beside `like` or numpy arrays, as
        `like` is; the names in skip stay None."""
        if _is_torch(like):
            import torch
            td = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32}
            return {k: None if k in skip else torch.empty(s, dtype=td[d], device=like.device) for k, s, d in spec}
        return {k: None if k in skip else np.empty(s, d) for k, s, d in spec}

    def _call(self, fn, B, inputs, spec, out, stream, scalars, refuse_copies):
        """fn(handle, B, *inputs, *scalars, *outputs, mode, stream): inputs the eight pairs of _solve_inputs, the outputs out[name]
        for spec's names in ABI order, scalars the doubles the box entries take between the two."""
        n_in = len(inputs)
        arrs = [a for a, _ in inputs] + [out[k] for k, _, _ in spec]
        shapes = [s for _, s in inputs] + [s for _, s, _ in spec]
        dts = [np.uint32 if i == 3 else self.np_dtype for i in range(n_in)] + [d for _, _, d in spec]      # 3: flags
        mode, ptrs, keep = self._prep(arrs, shapes, dts)
        if refuse_copies and mode == L.IGT_MEM_HOST:
            for (k, _, _), ptr in zip(spec, ptrs[n_in:]):
                if keep_is_copy(out[k], ptr):
                    raise ValueError(f'out[{k!r}] must be a contiguous array of the solver dtype')
        self._check(fn(self._h, B, *ptrs[:n_in], *(float(v) for v in scalars), *ptrs[n_in:], mode,
                       self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out

    def _call_solve(self, fn, B, inputs, out, stream, scalars=()):
        """One solve entry -> dict(x, u, cost, argmin, status): allocated like x0 unless the caller brought it; an output the
        marshalling had to copy is refused."""
        dt, N = self.np_dtype, self.N
        spec = (('x', (B, 7, N + 1), dt), ('u', (B, 2, N), dt), ('cost', (B,), dt), ('argmin', (B,), np.int32),
                ('status', (B,), np.int32))
        if out is None:
            out = self._new_out(spec, inputs[0][0])
        return self._call(fn, B, inputs, spec, out, stream, scalars, True)

    def _call_rollout(self, fn, B, inputs, want_X, want_U, stream, scalars=()):
        """One roll-out entry of every candidate -> dict(X | None, U | None, cost, viol), numpy: the public methods have refused
        tensors."""
        dt, N, Cn = self.np_dtype, self.N, self.C
        spec = (('X', (B, Cn, 7, N + 1), dt), ('U', (B, Cn, 2, N), dt), ('cost', (B, Cn), dt), ('viol', (B, Cn), np.uint32))
        out = self._new_out(spec, None, skip=('X',) * (not want_X) + ('U',) * (not want_U))
        return self._call(fn, B, inputs, spec, out, stream, scalars, False)

    # ------------------------------------------------------------------ the solve
    def solve(self, x0, u_prev, kparams, flags, obs_xy=None, tv_sv=None, enc=None, out=None, stream=None, u_ws=None):
        """x0[B,7] u_prev[B,2] kparams[B,3] flags[B] obs_xy[B,n_obs,2,N+1]
        -> dict(x[B,7,N+1], u[B,2,N], cost[B], argmin[B], status[B]).
        u_ws[B,2,N]: warm start (previous solution shifted by one step, utils.py:354-363), read where
        flags & IGT_FLAG_WARM; ramp-hold candidates are then centred on it instead of on u_prev."""
        B = int(x0.shape[0])
        host_polish = self.value_polish_iters if self.value_polish_driver == 'host' else 0
        if host_polish and _is_torch(x0):
            raise TypeError('value_polish_iters > 0 is driven from the host: solve() takes numpy arrays then, not device tensors '
                            '(and cannot be captured in a stream graph); set_value_polish(0) for the device-resident solve')
        inputs = self._solve_inputs(B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, (u_ws, (B, 2, self.N)))
        out = self._call_solve(self._solve, B, inputs, out, stream)
        if host_polish:      # (host arrays: the solve above has synchronised)
            self._value_polish_host(x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, out, host_polish)
        return out

    def rollout_all(self, x0, u_prev, kparams, flags, obs_xy=None, tv_sv=None, enc=None, want_X=True, want_U=True,
                    stream=None, u_ws=None):
        """Every candidate of every scenario (parity/debug):
        -> dict(X[B,C,7,N+1] | None, U[B,C,2,N] | None, cost[B,C], viol[B,C])."""
        B = int(x0.shape[0])
        if _is_torch(x0):
            raise TypeError('rollout_all is a host-mode debug entry (numpy buffers)')
        inputs = self._solve_inputs(B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, (u_ws, (B, 2, self.N)))
        return self._call_rollout(self._rollout, B, inputs, want_X, want_U, stream)

    # ------------------------------------------------------------------ per-scenario candidate sets
    def _check_candidates(self, what, x0, U):
        """What solve_candidates / rollout_candidates refuse before any GPU call; -> B."""
        if self.dtype != 'f64':
            raise ValueError(f"{what} needs dtype='f64' (the float kernels read a double table and would need a conversion pass)")
        if self.params.cand_mode != L.IGT_CAND_TABLE:
            raise ValueError(f"{what} needs cand_mode='table' (it fixes C and N; set_candidate_table need not be called)")
        B = int(x0.shape[0])
        want = (B, self.C, 2, self.N)
        if U is None or not hasattr(U, 'shape') or tuple(U.shape) != want:
            raise ValueError(f'U must be [B,C,2,N] = {want}, not {None if U is None else tuple(getattr(U, "shape", ()))}')
        return B

    def solve_candidates(self, x0, u_prev, kparams, flags, U, obs_xy=None, tv_sv=None, enc=None, out=None, stream=None):
        """solve() on candidates of the caller's, one set per scenario: U[B,C,2,N], scenario b's C control sequences (a_k, then
        df_k), judged like any table candidate -- rate limit and input box included (igtmpc.h igt_solve_candidates_f64).
        -> the dict of solve(); row b is, bit for bit, what a table solver whose shared table is U[b] answers for scenario b.
        float64 solvers with cand_mode='table'; numpy arrays or tensors on the solver's GPU, as solve -- with tensors the call only
        enqueues and can be captured, and a replay reads what U holds then.  polish_iters and the device-driven value polish act
        behind the emit as in solve(); the host-driven value polish is solve()'s own loop and is refused here."""
        B = self._check_candidates('solve_candidates', x0, U)
        if self.value_polish_iters > 0 and self.value_polish_driver == 'host':
            raise TypeError("value_polish_iters > 0 under value_polish_driver='host' is solve()'s loop: "
                            "set_value_polish_driver('device') takes the steps inside solve_candidates, set_value_polish(0) none")
        fn = self._entry('igt_solve_candidates_f64')
        inputs = self._solve_inputs(B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, (U, (B, self.C, 2, self.N)))
        return self._call_solve(fn, B, inputs, out, stream)

    def rollout_candidates(self, x0, u_prev, kparams, flags, U, obs_xy=None, tv_sv=None, enc=None, want_X=True, want_U=True,
                           stream=None):
        """rollout_all() on the per-scenario candidates U[B,C,2,N] of solve_candidates (igtmpc.h igt_rollout_candidates_f64):
        -> dict(X[B,C,7,N+1] | None, U[B,C,2,N] | None, cost[B,C], viol[B,C]).  Host mode, like rollout_all."""
        B = self._check_candidates('rollout_candidates', x0, U)
        if _is_torch(x0) or _is_torch(U):
            raise TypeError('rollout_candidates is a host-mode entry (numpy buffers), like rollout_all')
        fn = self._entry('igt_rollout_candidates_f64')
        inputs = self._solve_inputs(B, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, (U, (B, self.C, 2, self.N)))
        return self._call_rollout(fn, B, inputs, want_X, want_U, stream)

    # ------------------------------------------------------------------ rectangle (OBCA) collision model
    def _check_box(self, what, x0):
        """What solve_box / rollout_all_box refuse before any GPU call (the library refuses the rest, naming the cause); -> B."""
        if self.dtype != 'f64':
            raise ValueError(f"{what} needs dtype='f64' (there is no float32 entry for the rectangle collision model)")
        if self.value_polish_iters > 0:
            raise ValueError(f'{what}: value_polish_iters > 0 is not supported (the polish judges its trial plans with the '
                             f'circle); set_value_polish(0) for a box solve')
        return int(x0.shape[0])

    def solve_box(self, x0, u_prev, kparams, flags, obs_pose, tv_sv=None, enc=None, out=None, stream=None, u_ws=None,
                  length=4.47, width=2.0, d_box=0.0):
        """solve() under the rectangle (OBCA) collision model (igtmpc.h igt_solve_batch_box_f64): obs_pose[B,n_obs,3,N+1] holds
        the obstacles' x, y and heading; ego and obstacles are rectangles of length x width that must stay d_box + 1e-6 apart
        (the reference's 'obca' mode: 4.47 x 2.0, d_min = 0).  -> the dict of solve().  float64 solvers, any candidate family,
        both costs; numpy arrays or tensors on the solver's GPU, as solve -- with tensors the call only enqueues and can be
        captured.  Stateless: solve() of the same solver keeps judging circles.  Solvers with polish_iters > 0 or a value polish
        are refused."""
        B = self._check_box('solve_box', x0)
        fn = self._entry('igt_solve_batch_box_f64')
        inputs = self._solve_inputs(B, x0, u_prev, kparams, flags, obs_pose, tv_sv, enc, (u_ws, (B, 2, self.N)), obs_rows=3)
        return self._call_solve(fn, B, inputs, out, stream, scalars=(length, width, d_box))

    def rollout_all_box(self, x0, u_prev, kparams, flags, obs_pose, tv_sv=None, enc=None, want_X=True, want_U=True,
                        stream=None, u_ws=None, length=4.47, width=2.0, d_box=0.0):
        """rollout_all() under the rectangle collision model of solve_box (igtmpc.h igt_rollout_batch_box_f64):
        -> dict(X[B,C,7,N+1] | None, U[B,C,2,N] | None, cost[B,C], viol[B,C]); the collision bit is the rectangles'.
        Host mode, like rollout_all."""
        B = self._check_box('rollout_all_box', x0)
        if _is_torch(x0):
            raise TypeError('rollout_all_box is a host-mode entry (numpy buffers), like rollout_all')
        fn = self._entry('igt_rollout_batch_box_f64')
        inputs = self._solve_inputs(B, x0, u_prev, kparams, flags, obs_pose, tv_sv, enc, (u_ws, (B, 2, self.N)), obs_rows=3)
        return self._call_rollout(fn, B, inputs, want_X, want_U, stream, scalars=(length, width, d_box))

    # ------------------------------------------------------------------ polish under the value-network cost
    def _drop_vp_table(self):
        t, self._vp_table = getattr(self, '_vp_table', None), None
        if t is not None:
            t.close()

    def _vp_trial_handle(self):
        """A table handle (C = 64) with this solver's limits, terminal set and network: it rolls and judges the 64 trials.
        Built from self.params as igt_create took them (the library reads them once; changing the struct later changes neither
        handle) and dropped when set_cinf / set_value_net change what it mirrors.  A second copy of the network and a workspace
        of its own: the price of driving the steps from the host."""
        if self._vp_table is None:
            own = ('N', 'dt', 'n_rk4', 'C', 'n_obs', 'cand_mode', 'cost_mode', 'polish_iters', 'refine_iters')
            limits = {k: getattr(self.params, k) for k, _ in L.igt_params._fields_ if k not in own}
            t = BatchSolver(N=self.N, dt=self.params.dt, n_rk4=self.params.n_rk4, C=VALUE_POLISH_TRIALS, n_obs=self.n_obs,
                            device=self.device, dtype='f64', cand_mode='table', cost_mode='value_net', **limits)
            if self._cinf_args is not None:
                t.set_cinf(*self._cinf_args)
            t.set_value_net(*self._net_args)
            self._vp_table = t
        return self._vp_table

    def set_value_polish(self, k):
        """Projected-gradient steps that solve() takes on every solved scenario's winner under the value-network cost (0..4;
        0, the default: the solve as it is without this call, bit for bit).  float64 solvers with cost_mode='value_net';
        polish_iters, the progress cost's polish, keeps refusing the value network.  Who takes the steps is the solver's
        value_polish_driver (the keyword, or set_value_polish_driver): under 'host', the default, they are driven from numpy
        (_value_polish_host) -- solve() takes them for host arrays and refuses device tensors, and with them stream capture,
        with a TypeError while k > 0; under 'device' the library takes them inside the solve (igtmpc.h igt_set_value_polish: six
        launches an iteration on the solve's stream) for host arrays and device tensors alike -- a solve on a capturing stream is
        then refused by the library (IgtError, 'stream capture')."""
        self._set_value_polish(k, self.value_polish_driver)

    def set_value_polish_driver(self, driver):
        """'host' or 'device' (see set_value_polish); the number of iterations stays as it is."""
        self._set_value_polish(self.value_polish_iters, driver)

    def _set_value_polish(self, k, driver):
        check_value_polish(k, self.dtype, self.cost_mode)
        check_value_polish_driver(driver)
        field = int(k) if driver == 'device' else 0
        if field != self._vp_field:      # (a library from before the entry serves the 'host' driver and k = 0)
            self._check(self._entry('igt_set_value_polish')(self._h, field))
            self._vp_field = field
        self.value_polish_iters, self.value_polish_driver = int(k), driver

    def _value_polish_host(self, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, out, iters):
        """Projected-gradient steps on every solved scenario's winner under the value-network cost (gt_mpc, mpc.py:356-369), driven
        from the host through device entries that exist, in place in out = the solve's result for the same inputs (host
        arrays).  Per solved scenario and iteration, from the plan u [2, N] and its cost J0 (iteration 1: the solve's):
          1. g = dJ/du by igt_cost_gradient_vn_f64 at the plan (the costate seeded with the network's partials at the plan's own
             (s_N, v_N)); non-finite entries become 0;
          2. d = -g / scale, scale = max(max|g_a| / (4 dt jerk), max|g_df| / (4 dt steer_rate)) + 1e-30; steer_rate = 0: the
             steering row of d is 0;
          3. 64 trials u + 2^(-m/3) d, clamped step by step to the rate window around the clamped step before it, then to the box,
             rolled, judged by every verdict and priced (stage terms - V_out of the trial's own terminal state) by
             igt_rollout_batch_f64 on a table handle of 64 candidates with this solver's limits, terminal set and network;
          4. the feasible trial of least cost, ties to the lowest m, accepted only if strictly cheaper than J0; else the scenario
             stops for good.
        x is the accepted trial's own table roll-out, cost never rises, argmin, status and unsolved rows are the solve's.  One gradient
        launch per iteration for the whole batch, one table upload and roll-out per scenario and iteration: made for the
        planner's one problem and for batches of some hundreds, with a host synchronisation per call (profiles/
        value_polish_host_time.txt has the cost per scenario and iteration)."""
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        x0, u_prev, kparams, obs_xy, tv_sv, enc = (f8(a) for a in (x0, u_prev, kparams, obs_xy, tv_sv, enc))
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        p, N = self.params, self.N
        ra, rd = p.dt * p.jerk_limit, p.dt * p.steer_rate_limit
        alpha = 2.0 ** (-np.arange(VALUE_POLISH_TRIALS) / 3.0)
        table = self._vp_trial_handle()
        alive = np.flatnonzero(out['status'] == 0)
        for _ in range(iters):
            if len(alive) == 0:
                break
            g = self.cost_gradient(x0[alive], kparams[alive], flags[alive], f8(out['u'][alive]), tv_sv=tv_sv[alive],
                                   enc=enc[alive])['grad']
            g = np.where(np.isfinite(g), g, 0.0)
            ma, md = np.abs(g[:, 0]).max(axis=-1), np.abs(g[:, 1]).max(axis=-1)
            scale = (np.maximum(ma / (4 * ra), md / (4 * rd)) if rd > 0 else ma / (4 * ra)) + 1e-30
            d = -g / scale[:, None, None]
            if not rd > 0:
                d[:, 1] = 0.0
            keep = []
            for i, b in enumerate(alive):
                U = out['u'][b][None] + alpha[:, None, None] * d[i][None]          # [64, 2, N]
                pa = np.full(VALUE_POLISH_TRIALS, u_prev[b, 0])
                pd = np.full(VALUE_POLISH_TRIALS, u_prev[b, 1])
                for k in range(N):
                    pa = np.clip(np.clip(U[:, 0, k], pa - ra, pa + ra), p.a_min, p.a_max)
                    pd = np.clip(np.clip(U[:, 1, k], pd - rd, pd + rd), -p.df_max, p.df_max)
                    U[:, 0, k], U[:, 1, k] = pa, pd
                table.set_candidate_table(U)
                r = table.rollout_all(x0[b:b + 1], u_prev[b:b + 1], kparams[b:b + 1], flags[b:b + 1], obs_xy[b:b + 1],
                                      tv_sv[b:b + 1], enc[b:b + 1], want_U=False)
                J = np.where((r['viol'][0] == 0) & np.isfinite(r['cost'][0]), r['cost'][0], np.inf)
                m = int(J.argmin())                                                 # first minimum: the lowest m
                if J[m] < out['cost'][b]:
                    out['u'][b], out['x'][b], out['cost'][b] = U[m], r['X'][0, m], J[m]
                    keep.append(b)
            alive = np.asarray(keep, dtype=np.int64)

    def _entry(self, name):
        """An entry added without a change of IGT_VERSION: a library from before it (IGT_LIB_PATH) does not export it."""
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise L.IgtError(f'this libigtmpc.so does not export {name}: it was built before the entry was added; rebuild it '
                             f'(`make -C igt-mpc-int_amd/csrc`)')
        return fn

    def terminal_value(self, sv, tv_sv, enc, want_grad=True, out=None, stream=None):
        """The terminal term of the gt_mpc cost, V(Wn (x_N - mu_f)) sigma_t + mu_t (mpc.py:326-338, 369), for n terminal ego states
        of their own scenarios and -- want_grad -- its partials by (s_N, v_N) (igtmpc.h igt_terminal_value_f64):
        sv[n,2] = (s_N, v_N), tv_sv[n,2], enc[n,2] -> dict(V[n], dV[n,2] | None).  float64 solvers with cost_mode='value_net' and a
        network set; numpy arrays or tensors on the solver's GPU, as solve."""
        if self.dtype != 'f64':
            raise ValueError("terminal_value needs dtype='f64'")
        fn = self._entry('igt_terminal_value_f64')
        n = int(sv.shape[0])
        if out is None:
            if _is_torch(sv):
                import torch
                out = dict(V=torch.empty((n,), dtype=torch.float64, device=sv.device),
                           dV=torch.empty((n, 2), dtype=torch.float64, device=sv.device) if want_grad else None)
            else:
                out = dict(V=np.empty((n,), np.float64), dV=np.empty((n, 2), np.float64) if want_grad else None)
        f8 = np.float64
        dV = out.get('dV') if want_grad else None
        if want_grad and dV is None:
            raise ValueError("want_grad=True needs out['dV']")
        mode, ptrs, keep = self._prep([sv, tv_sv, enc, out['V'], dV], [(n, 2), (n, 2), (n, 2), (n,), (n, 2)], [f8] * 5)
        if mode == L.IGT_MEM_HOST:
            for k, i in (('V', 3), ('dV', 4)):
                if ptrs[i] is not None and keep_is_copy(out[k], ptrs[i]):
                    raise ValueError(f'out[{k!r}] must be a contiguous float64 array')
        self._check(fn(self._h, n, *ptrs, mode, self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out

    def cost_gradient(self, x0, kparams, flags, U, out=None, stream=None, tv_sv=None, enc=None):
        """dJ/du of the progress cost (mpc.py:356-373) for one control sequence per scenario, no projection and no verdicts
        (igtmpc.h igt_cost_gradient_f64): x0[B,7] kparams[B,3] flags[B] U[B,2,N] -> dict(cost[B], grad[B,2,N]); a non-finite
        cost gives a NaN row.  float64 solvers with the progress cost; numpy arrays or tensors on the solver's GPU, as solve.
        With tv_sv[B,2] and enc[B,2] on a cost_mode='value_net' solver: the same for the value-network cost, whose terminal term
        is -terminal_value(s_N, v_N) (igtmpc.h igt_cost_gradient_vn_f64)."""
        if self.dtype != 'f64':
            raise ValueError("cost_gradient needs dtype='f64'")
        B, N = int(x0.shape[0]), self.N
        if tv_sv is not None and enc is not None and self.params.cost_mode == L.IGT_COST_VALUE_NET:
            return self._cost_gradient_vn(B, x0, kparams, flags, tv_sv, enc, U, out, stream)
        torch_mode = _is_torch(x0)
        if out is None:
            if torch_mode:
                import torch
                out = dict(cost=torch.empty((B,), dtype=torch.float64, device=x0.device),
                           grad=torch.empty((B, 2, N), dtype=torch.float64, device=x0.device))
            else:
                out = dict(cost=np.empty((B,), np.float64), grad=np.empty((B, 2, N), np.float64))
        f8 = np.float64
        mode, ptrs, keep = self._prep([x0, kparams, flags, U, out['cost'], out['grad']],
                                      [(B, 7), (B, 3), (B,), (B, 2, N), (B,), (B, 2, N)], [f8, f8, np.uint32, f8, f8, f8])
        if mode == L.IGT_MEM_HOST:
            for k, i in (('cost', 4), ('grad', 5)):
                if keep_is_copy(out[k], ptrs[i]):
                    raise ValueError(f'out[{k!r}] must be a contiguous float64 array')
        self._check(self.lib.igt_cost_gradient_f64(self._h, B, *ptrs, mode, self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out

    def _cost_gradient_vn(self, B, x0, kparams, flags, tv_sv, enc, U, out, stream):
        fn = self._entry('igt_cost_gradient_vn_f64')
        N = self.N
        if out is None:
            if _is_torch(x0):
                import torch
                out = dict(cost=torch.empty((B,), dtype=torch.float64, device=x0.device),
                           grad=torch.empty((B, 2, N), dtype=torch.float64, device=x0.device))
            else:
                out = dict(cost=np.empty((B,), np.float64), grad=np.empty((B, 2, N), np.float64))
        f8 = np.float64
        mode, ptrs, keep = self._prep([x0, kparams, flags, tv_sv, enc, U, out['cost'], out['grad']],
                                      [(B, 7), (B, 3), (B,), (B, 2), (B, 2), (B, 2, N), (B,), (B, 2, N)],
                                      [f8, f8, np.uint32, f8, f8, f8, f8, f8])
        if mode == L.IGT_MEM_HOST:
            for k, i in (('cost', 6), ('grad', 7)):
                if keep_is_copy(out[k], ptrs[i]):
                    raise ValueError(f'out[{k!r}] must be a contiguous float64 array')
        self._check(fn(self._h, B, *ptrs, mode, self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out

    def set_routes(self, table=None):
        """Route geometry for forecast(); default: the four-way intersection of igtmpc.routes."""
        if table is None:
            from . import routes as R
            T = R.TABLES
            table = np.column_stack([T['p0'], T['t'], T['c'], T['b0'], T['b1'], T['R'], T['end'],
                                     (T['turn'] == 0).astype(np.float64)])
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 12:
            raise ValueError('route table must be [n_routes, 12]')
        self._check(self.lib.igt_set_routes(self._h, len(table), table.ctypes.data))
        self._routes_set = True
        if len(table) != self._n_routes:      # the library drops the headings of a table of another length
            self._headings_set = False
        self._n_routes = len(table)

    def forecast(self, ego_xyh, opp, opp_a, opp_route, plan_x=None, plan_u=None, has_plan=None, stream=None):
        """Opponent forecast + V2V sharing + filter_preds on the device (constant_acceleration_model.py:18-82,
        utils.py:339-352, 365-388): -> (obs_xy[B,n_obs,2,N+1], tv_sv[B,2]).
        Two-vehicle scenes (n_obs = 1): opp[B,4], opp_a[B], opp_route[B], plan_x[B,7,N+1], plan_u[B,2,N], has_plan[B].
        M > 2 (mpc.py:82-83 takes any M): the same arrays with an n_obs axis behind B -- opp[B,n_obs,4], opp_a[B,n_obs], ... -- and
        tv_sv[B,n_obs,2] (the last raw prediction of every other vehicle, mpc.py:263-276)."""
        if not self._routes_set:
            self.set_routes()
        return self._forecast_gathered(self._fcast, 2, ego_xyh, opp, opp_a, opp_route, (), plan_x, plan_u, has_plan, stream)

    def _call_forecast(self, fn, count, inputs, obs_shape, tv_shape, stream):
        """One forecast entry: fn(handle, count, *inputs, obs, tv, mode, stream) with inputs = (array, shape, dtype) in ABI order
        -> (obs, tv), allocated like the first input."""
        dt = self.np_dtype
        spec = (('obs', obs_shape, dt), ('tv', tv_shape, dt))
        out = self._new_out(spec, inputs[0][0])
        arrs, shapes, dts = zip(*inputs, *((out[k], s, d) for k, s, d in spec))
        mode, ptrs, keep = self._prep(arrs, shapes, dts)
        self._check(fn(self._h, count, *ptrs, mode, self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out['obs'], out['tv']

    def _forecast_gathered(self, fn, rows, ego_xyh, opp, opp_a, opp_route, heading, plan_x, plan_u, has_plan, stream):
        """forecast (rows = 2, heading = ()) and forecast_pose (rows = 3, heading = (opp_heading,)): one problem per ego."""
        B, N, M1, dt = int(ego_xyh.shape[0]), self.N, self.n_obs, self.np_dtype
        ax = () if M1 == 1 else (M1,)
        inputs = [(ego_xyh, (B, 3), dt), (opp, (B, *ax, 4), dt), (opp_a, (B, *ax), dt), (opp_route, (B, *ax), np.int32),
                  *((h, (B, *ax), dt) for h in heading),
                  (plan_x, (B, *ax, 7, N + 1), dt), (plan_u, (B, *ax, 2, N), dt), (has_plan, (B, *ax), np.int32)]
        return self._call_forecast(fn, B, inputs, (B, M1, rows, N + 1), (B, *ax, 2), stream)

    def _forecast_scenes(self, fn, rows, x, a_prev, route, plan_x, plan_u, has_plan, stream):
        """forecast_scene (rows = 2) and forecast_scene_pose (rows = 3): E scenes of M agents, one row per agent."""
        E, N, M, dt = int(x.shape[0]), self.N, self.n_obs + 1, self.np_dtype
        inputs = [(x, (E, M, 7), dt), (a_prev, (E, M), dt), (route, (E, M), np.int32), (plan_x, (E, M, 7, N + 1), dt),
                  (plan_u, (E, M, 2, N), dt), (has_plan, (E, M), np.int32)]
        return self._call_forecast(fn, E, inputs, (E * M, M - 1, rows, N + 1), (E * M, M - 1, 2), stream)

    def forecast_scene(self, x, a_prev, route, plan_x=None, plan_u=None, has_plan=None, stream=None):
        """forecast() for E whole scenes of M = n_obs + 1 agents, scene-major, nothing gathered (igt_forecast_scene_*):
        x[E,M,7] (planner state order), a_prev[E,M], route[E,M], plan_x[E,M,7,N+1], plan_u[E,M,2,N], has_plan[E,M]
        -> (obs_xy[E M,n_obs,2,N+1], tv_sv[E M,n_obs,2]) -- problem e M + i is agent i of scene e as ego, its opponents the
        other agents in ascending order.  Each agent is forecast once and filtered per ego; equals forecast() on the gathered
        inputs bit for bit."""
        if not self._routes_set:
            self.set_routes()
        return self._forecast_scenes(self._fscene, 2, x, a_prev, route, plan_x, plan_u, has_plan, stream)

    # ------------------------------------------------------------------ pose forecast (x, y, heading: what solve_box reads)
    def set_route_headings(self, table=None):
        """Route headings for forecast_scene_pose() / forecast_pose() (igtmpc.h igt_set_route_headings): table[n_routes,3] =
        (h0, hN, abs) per route of the set_routes table; default: those of igtmpc.routes.  The route table is set first if it is
        not yet."""
        self._check_pose('set_route_headings')
        if not self._routes_set:
            self.set_routes()
        if table is None:
            from . import routes as R
            T = R.TABLES
            table = np.column_stack([T['h0'], T['hN'], T['abs_heading'].astype(np.float64)])
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 3:
            raise ValueError('route heading table must be [n_routes, 3]')
        self._check(self._entry('igt_set_route_headings')(self._h, len(table), table.ctypes.data))
        self._headings_set = True

    def _check_pose(self, what):
        """What the pose entries refuse before any library call."""
        if self.dtype != 'f64':
            raise ValueError(f"{what} needs dtype='f64' (the pose is read by solve_box, which has no float32 entry)")

    def forecast_scene_pose(self, x, a_prev, route, plan_x=None, plan_u=None, has_plan=None, stream=None):
        """forecast_scene() with the obstacles' headings (igtmpc.h igt_forecast_scene_pose_f64): the same arguments
        -> (obs_pose[E M,n_obs,3,N+1], tv_sv[E M,n_obs,2]).  Rows 0, 1 and tv_sv are forecast_scene()'s, bit for bit; row 2 is
        every other agent's heading along its forecast (node 0: its true heading x[e,j,6]; then the route's reference heading at
        the forecast's arc length) or along the plan it shares (plan_x[e,j,6,1:], then the route heading one predicted step behind
        the plan's end), |heading| on the routes that read it so -- not filtered: an agent behind the ego keeps its heading row.
        float64 solvers; numpy arrays or tensors on the solver's GPU -- with tensors the call only enqueues and can be captured."""
        self._check_pose('forecast_scene_pose')
        if not self._headings_set:
            self.set_route_headings()
        fn = self._entry('igt_forecast_scene_pose_f64')
        return self._forecast_scenes(fn, 3, x, a_prev, route, plan_x, plan_u, has_plan, stream)

    def forecast_pose(self, ego_xyh, opp, opp_a, opp_route, opp_heading, plan_x=None, plan_u=None, has_plan=None, stream=None):
        """forecast() with the obstacles' headings, per gathered problem (igtmpc.h igt_forecast_batch_pose_f64): forecast()'s
        arguments plus opp_heading[B] ([B,n_obs] for n_obs > 1), every opponent's true heading
        -> (obs_pose[B,n_obs,3,N+1], tv_sv[B,2] or [B,n_obs,2]).  forecast_scene_pose() equals it on the gathered inputs bit for
        bit."""
        self._check_pose('forecast_pose')
        if not self._headings_set:
            self.set_route_headings()
        fn = self._entry('igt_forecast_batch_pose_f64')
        return self._forecast_gathered(fn, 3, ego_xyh, opp, opp_a, opp_route, (opp_heading,), plan_x, plan_u, has_plan, stream)

    def frenet_step(self, x, u, kparams, stream=None):
        """One control step of the RK4 Frenet model for n states: x[n,7], u[n,2], kparams[n,3]
        -> x_next[n,7]   (kinematic_bicycle_model_frenet.py:70-127)."""
        n = int(x.shape[0])
        dt = self.np_dtype
        if _is_torch(x):
            import torch
            out = torch.empty((n, 7), dtype=x.dtype, device=x.device)
        else:
            out = np.empty((n, 7), dt)
        mode, ptrs, keep = self._prep([x, u, kparams, out], [(n, 7), (n, 2), (n, 3), (n, 7)], [dt] * 4)
        self._check(self._fstep(self._h, n, *ptrs, mode, self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out

    def loop_advance(self, x, u_prev, kparams, status, x_sol, u_sol, a_brake, flags=None, infeasible=None, x_log=None,
                     u_log=None, step=None, want_ws=True, out=None, stream=None):
        """The closed-loop step behind a solve, in one kernel (igtmpc.h igt_loop_advance_*; evaluate.py:491-545): per agent,
        apply the first control of a solved problem or take the brake fallback (deceleration a_brake), and leave what the next
        forecast and solve read.  n = E M agents in the solve's row order.
        x[n,7], u_prev[n,2] (float64) are UPDATED IN PLACE; kparams[n,3] (float64); status[n], x_sol[n,7,N+1], u_sol[n,2,N]: the
        solve's out['status'], out['x'], out['u'] (the solver's dtype)
        -> dict(has_plan[n] int32, plan_x[n,7,N+1], plan_u[n,2,N], u_ws[n,2,N] | None (want_ws=False), flags[n] | None);
        `out` may bring those buffers (a captured step writes the same ones every replay).
        flags[n]: out['flags'] = flags | IGT_FLAG_WARM where solved -- with u_ws the next solve's warm start.
        infeasible[n] (int64): += 1 where not solved, in place.  x_log[n,7,T+1], u_log[n,2,T] (float64) with step (an int64
        tensor of one element on the device; host mode: an int): u_log[:,:,step] and x_log[:,:,step+1] are written in place,
        a step outside 0..T-1 writes nothing.  numpy arrays or tensors on the solver's GPU, as solve."""
        fn = self._entry(f'igt_loop_advance_{self.dtype}')
        n, N, dt, f8 = int(x.shape[0]), self.N, self.np_dtype, np.float64
        torch_mode = _is_torch(x)
        if (x_log is None) != (u_log is None):
            raise ValueError('x_log and u_log go together')
        if x_log is not None and step is None:
            raise ValueError('logging needs step')
        T_log = int(u_log.shape[2]) if u_log is not None else 0
        if step is not None and not torch_mode and not isinstance(step, np.ndarray):
            step = np.array([int(step)], dtype=np.int64)
        if x_log is None:
            step = None
        out = dict(out or {})
        if torch_mode:
            import torch
            td = torch.float32 if self.dtype == 'f32' else torch.float64
            new = lambda shp, d: torch.empty(shp, dtype=d, device=x.device)
            i32, u32 = torch.int32, torch.int32
        else:
            td, new, i32, u32 = dt, lambda shp, d: np.empty(shp, d), np.int32, np.uint32
        out.setdefault('has_plan', new((n,), i32))
        out.setdefault('plan_x', new((n, 7, N + 1), td))
        out.setdefault('plan_u', new((n, 2, N), td))
        if want_ws:
            out.setdefault('u_ws', new((n, 2, N), td))
        else:
            out['u_ws'] = None
        if flags is not None:
            out.setdefault('flags', new((n,), u32))
        else:
            out['flags'] = None
        arrs = [x, u_prev, kparams, status, x_sol, u_sol, out['has_plan'], out['plan_x'], out['plan_u'], out['u_ws'], flags,
                out['flags'], infeasible, x_log, u_log, step]
        shapes = [(n, 7), (n, 2), (n, 3), (n,), (n, 7, N + 1), (n, 2, N), (n,), (n, 7, N + 1), (n, 2, N), (n, 2, N), (n,), (n,),
                  (n,), (n, 7, T_log + 1), (n, 2, T_log), (1,)]
        dts = [f8, f8, f8, np.int32, dt, dt, np.int32, dt, dt, dt, np.uint32, np.uint32, np.int64, f8, f8, np.int64]
        mode, p, keep = self._prep(arrs, shapes, dts)
        if mode == L.IGT_MEM_HOST:
            written = dict(x=(x, 0), u_prev=(u_prev, 1), has_plan=(out['has_plan'], 6), plan_x=(out['plan_x'], 7),
                           plan_u=(out['plan_u'], 8), u_ws=(out['u_ws'], 9), flags=(out['flags'], 11), infeasible=(infeasible, 12),
                           x_log=(x_log, 13), u_log=(u_log, 14))
            for k, (a, i) in written.items():
                if a is not None and keep_is_copy(a, p[i]):
                    raise ValueError(f'{k} is written in place: it must be a contiguous array of its dtype')
        self._check(fn(self._h, n, *p[:6], float(a_brake), *p[6:], T_log, mode, self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out

    def cartesian_euler(self, z0, u, stream=None):
        """z0[n,4]=(x,y,psi,v), u[n,2,T] -> z[n,4,T+1]   (kinematic_bicycle_model.py:15-50)."""
        n, T = int(z0.shape[0]), int(u.shape[2])
        dt = self.np_dtype
        if _is_torch(z0):
            import torch
            out = torch.empty((n, 4, T + 1), dtype=z0.dtype, device=z0.device)
        else:
            out = np.empty((n, 4, T + 1), dt)
        mode, ptrs, keep = self._prep([z0, u, out], [(n, 4), (n, 2, T), (n, 4, T + 1)], [dt, dt, dt])
        self._check(self._cart(self._h, n, T, *ptrs, mode, self._stream_ptr(stream, mode == L.IGT_MEM_DEVICE)))
        return out


def keep_is_copy(arr, ptr):
    """True when np.ascontiguousarray had to copy an OUTPUT buffer (results would be lost)."""
    return isinstance(arr, np.ndarray) and arr.ctypes.data != ptr
