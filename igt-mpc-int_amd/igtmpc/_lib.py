"""ctypes binding of include/igtmpc.h (libigtmpc.so, built by csrc/Makefile).

The product path has no CPU fallback: if the HIP library is missing or fails to
load, importing a solver raises ImportError with the build command."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libigtmpc.so')

IGT_MEM_DEVICE, IGT_MEM_HOST = 0, 1
IGT_CAND_LATTICE, IGT_CAND_TABLE, IGT_CAND_RAMP_HOLD, IGT_CAND_TRACK = 0, 1, 2, 3
IGT_COST_PROGRESS, IGT_COST_VALUE_NET = 0, 1
IGT_FLAG_ABS_HEADING = 1
IGT_FLAG_WARM = 2
IGT_GRAD_FORWARD_DIFF, IGT_GRAD_ADJOINT = 0, 1
IGT_POLISH_STEP_GRADIENT, IGT_POLISH_STEP_NEWTON = 0, 1
VIOL_BITS = dict(box_v=1, box_u=2, rate=4, ey=8, terminal=16, collision=32, nonfinite=64)


class igt_params(C.Structure):
    _fields_ = [('N', C.c_int32), ('n_rk4', C.c_int32), ('C', C.c_int32), ('n_obs', C.c_int32),
                ('cand_mode', C.c_int32), ('cost_mode', C.c_int32),
                ('dt', C.c_double), ('l_r', C.c_double), ('l_f', C.c_double),
                ('v_min', C.c_double), ('v_max', C.c_double), ('a_min', C.c_double), ('a_max', C.c_double),
                ('df_max', C.c_double), ('jerk_limit', C.c_double), ('steer_rate_limit', C.c_double),
                ('ey_lim', C.c_double), ('d_min', C.c_double), ('w_u', C.c_double), ('feas_tol', C.c_double),
                ('refine_iters', C.c_int32), ('polish_iters', C.c_int32),
                ('track_ke', C.c_double), ('track_span', C.c_double), ('track_beta_lim', C.c_double),
                ('track_env', C.c_double), ('track_vcap', C.c_double)]


# every symbol include/igtmpc.h declares: name -> (restype, argtypes)
_vp, _i32, _i = C.c_void_p, C.c_int32, C.c_int
_SOLVE = [_vp, _i32] + [_vp] * 12 + [_i, _vp]
_ROLL = [_vp, _i32] + [_vp] * 11 + [_i, _vp]
_SOLVE_WS = [_vp, _i32] + [_vp] * 13 + [_i, _vp]
_ROLL_WS = [_vp, _i32] + [_vp] * 12 + [_i, _vp]
_CART = [_vp, _i32, _i32, _vp, _vp, _vp, _i, _vp]
_FSTEP = [_vp, _i32, _vp, _vp, _vp, _vp, _i, _vp]
_FCAST = [_vp, _i32] + [_vp] * 9 + [_i, _vp]
_FSCENE = [_vp, _i32] + [_vp] * 8 + [_i, _vp]
# x, u_prev, kparams, status, x_sol, u_sol | a_brake | has_plan, plan_x, plan_u, u_ws, flags_in, flags_out, infeasible, x_log, u_log, step | T_log
_LOOP = [_vp, _i32] + [_vp] * 6 + [C.c_double] + [_vp] * 10 + [_i32, _i, _vp]
SYMBOLS = {
    'igt_version': (_i, []),
    'igt_last_error': (C.c_char_p, []),
    'igt_params_default': (_i, [C.POINTER(igt_params)]),
    'igt_create': (_i, [C.POINTER(igt_params), _i, C.POINTER(_vp)]),
    'igt_destroy': (_i, [_vp]),
    'igt_get_params': (_i, [_vp, C.POINTER(igt_params)]),
    'igt_set_cinf': (_i, [_vp, _vp, _vp, _i32]),
    'igt_set_candidate_table': (_i, [_vp, _vp]),
    'igt_set_value_net': (_i, [_vp, _i32, _vp, _vp, _vp, _vp, C.c_double, C.c_double]),
    'igt_solve_batch_f32': (_i, _SOLVE),
    'igt_solve_batch_f64': (_i, _SOLVE),
    'igt_solve_batch_ws_f32': (_i, _SOLVE_WS),
    'igt_solve_batch_ws_f64': (_i, _SOLVE_WS),
    'igt_rollout_batch_f32': (_i, _ROLL),
    'igt_rollout_batch_f64': (_i, _ROLL),
    'igt_rollout_batch_ws_f32': (_i, _ROLL_WS),
    'igt_rollout_batch_ws_f64': (_i, _ROLL_WS),
    'igt_set_routes': (_i, [_vp, _i32, _vp]),
    'igt_forecast_batch_f32': (_i, _FCAST),
    'igt_forecast_batch_f64': (_i, _FCAST),
    'igt_forecast_scene_f32': (_i, _FSCENE),
    'igt_forecast_scene_f64': (_i, _FSCENE),
    'igt_frenet_step_f32': (_i, _FSTEP),
    'igt_frenet_step_f64': (_i, _FSTEP),
    'igt_cartesian_euler_f32': (_i, _CART),
    'igt_cartesian_euler_f64': (_i, _CART),
    'igt_comm_unique_id': (_i, [_vp]),
    'igt_comm_init': (_i, [_vp, _i32, _i32, _vp]),
    'igt_comm_destroy': (_i, [_vp]),
    'igt_allgather_controls_f32': (_i, [_vp, _i32, _vp, _vp, _vp]),
    'igt_allgather_controls_f64': (_i, [_vp, _i32, _vp, _vp, _vp]),
    'igt_set_concurrency': (_i, [_vp, _i32]),
    'igt_set_polish_gradient': (_i, [_vp, _i]),
    'igt_set_polish_step': (_i, [_vp, _i]),
    'igt_set_value_polish': (_i, [_vp, _i]),
    'igt_cost_gradient_f64': (_i, [_vp, _i32] + [_vp] * 6 + [_i, _vp]),
    'igt_terminal_value_f64': (_i, [_vp, _i32] + [_vp] * 5 + [_i, _vp]),
    'igt_cost_gradient_vn_f64': (_i, [_vp, _i32] + [_vp] * 8 + [_i, _vp]),
    'igt_solve_candidates_f64': (_i, _SOLVE_WS),       # U[B,C,2,N] where the _ws entries take u_ws
    'igt_rollout_candidates_f64': (_i, _ROLL_WS),
    # obs_pose[B,n_obs,3,N+1] where the _ws entries take obs_xy; length, width, d_box behind u_ws
    'igt_solve_batch_box_f64': (_i, [_vp, _i32] + [_vp] * 8 + [C.c_double] * 3 + [_vp] * 5 + [_i, _vp]),
    'igt_rollout_batch_box_f64': (_i, [_vp, _i32] + [_vp] * 8 + [C.c_double] * 3 + [_vp] * 4 + [_i, _vp]),
    'igt_set_route_headings': (_i, [_vp, _i32, _vp]),
    'igt_forecast_scene_pose_f64': (_i, _FSCENE),         # obs_pose[E M,n_obs,3,N+1] where the scene forecast takes obs_xy
    'igt_forecast_batch_pose_f64': (_i, [_vp, _i32] + [_vp] * 10 + [_i, _vp]),      # opp_heading behind opp_route
    'igt_loop_advance_f64': (_i, _LOOP),
    'igt_loop_advance_f32': (_i, _LOOP),
    'igt_set_profiling': (_i, [_vp, _i]),
    'igt_get_kernel_ms': (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'igt_algorithmic_bytes_per_solve': (_i, [_vp, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

# added without a change of IGT_VERSION: a library of the same ABI from before them (IGT_LIB_PATH, tools/ab_lib.sh) lacks them
OPTIONAL_SYMBOLS = ('igt_set_polish_gradient', 'igt_cost_gradient_f64', 'igt_terminal_value_f64', 'igt_cost_gradient_vn_f64',
                    'igt_set_polish_step', 'igt_set_value_polish', 'igt_solve_candidates_f64', 'igt_rollout_candidates_f64',
                    'igt_loop_advance_f64', 'igt_loop_advance_f32', 'igt_solve_batch_box_f64', 'igt_rollout_batch_box_f64',
                    'igt_set_route_headings', 'igt_forecast_scene_pose_f64', 'igt_forecast_batch_pose_f64')

_libs = {}
# IGT_DEV_FLAGS bits (csrc/igt_device.h DevFlag; the launch-time bits there are the library's own and not listed here)
DEV_NO_SLICES = 1
DEV_NO_EARLY_EXIT = 2
DEV_NO_STEER_TABLE = 4
DEV_NO_QUEUE_ORDER = 16
DEV_WAVES3 = 32
DEV_WIDE_ROWS = 64
DEV_EMIT_PRIO0 = 128
DEV_TRACE = 256
DEV_NO_STEAL = 512
DEV_EXACT64 = 1024
DEV_LITERAL = 2048
DEV_LATE_ITEMS = 15 << 12
DEV_NO_FAR = 65536
DEV_NO_PRUNE = 131072
DEV_STEER_SLICES = 262144
DEV_NO_CAPTURE = 524288
DEV_KEEP_QUEUES = 1048576
DEV_ALL_ROWS = 2097152
DEV_WHOLE_COLUMNS = 4194304
DEV_NO_BOUND = 8388608
DEV_NO_SEG_EMIT = 16777216
DEV_SEPARATE_QUEUES = 33554432
DEV_NO_REFILL = 1 << 26
DEV_NO_RESERVE = 1 << 27
DEV_KERNEL_FLAGS = DEV_WAVES3 | DEV_EXACT64 | DEV_LITERAL      # the kernels only libigtmpc_dev.so carries
LIB_PATH_DEV = os.path.join(os.path.dirname(LIB_PATH), 'libigtmpc_dev.so')


def wants_dev_kernels():
    """True when IGT_DEV_FLAGS (read by the library at igt_create) selects kernels only libigtmpc_dev.so carries."""
    try:
        return bool(int(os.environ.get('IGT_DEV_FLAGS', '0') or 0) & DEV_KERNEL_FLAGS)
    except ValueError:
        return False


def load(dev=None):
    """Loads libigtmpc.so (the shipped library) once and sets every prototype.  Raises ImportError when the library is
    absent -- there is deliberately no fallback path.  dev=True, or dev=None with IGT_DEV_FLAGS asking for developer
    kernels: libigtmpc_dev.so, the same sources built with IGT_DEV_KERNELS=1 (tests and A/B tools only)."""
    if dev is None:
        dev = wants_dev_kernels()
    dev = bool(dev)
    if dev in _libs:
        return _libs[dev]
    path = LIB_PATH_DEV if dev else LIB_PATH
    if not dev and os.environ.get('IGT_LIB_PATH'):      # A/B runs against another build of the same ABI (tools/ab_lib.sh)
        path = os.environ['IGT_LIB_PATH']
    if not os.path.exists(path):
        raise ImportError(f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          f'or `make -C igt-mpc-int_amd/csrc`')
    try:
        # torch ships its own libamdhip64; it must be the first HIP runtime the process
        # maps, otherwise a later `import torch` finds "No HIP GPUs" (two runtimes).
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise ImportError(f'cannot load {path}: {e}') from e
    for name, (res, args) in SYMBOLS.items():
        if name in OPTIONAL_SYMBOLS and path != (LIB_PATH_DEV if dev else LIB_PATH) and not hasattr(lib, name):
            continue                # an older build given by IGT_LIB_PATH: whoever needs the symbol gets the AttributeError
        fn = getattr(lib, name)     # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _libs[dev] = lib
    return lib


class IgtError(RuntimeError):
    pass


def check(rc, lib=None):
    if rc != 0:
        msg = (lib or load(False)).igt_last_error()
        raise IgtError(f'igtmpc error {rc}: {msg.decode() if msg else "?"}')
