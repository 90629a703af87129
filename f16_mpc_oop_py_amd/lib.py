"""ctypes binding of libf16hip.so (the C-ABI declared in include/f16_hip.h).

This is the same mechanism the reference uses for its plant: `ctypes.CDLL(<.so>)`
(parameters.py:108-114).  There is no CPU fallback: if the HIP library is missing or no GPU
is visible every entry point raises.
"""
import ctypes
import os
import subprocess

from . import cabi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO_PATH = os.environ.get("F16HIP_SO", os.path.join(HERE, "libf16hip.so"))   # override only for A/B experiments
SOURCES = ["f16_api.hip", "f16_dynamics.hip", "f16_control.hip", "f16_mpc_solve.hip", "f16_mpc_wave.hip", "f16_mpc_big.hip", "f16_trim.hip", "f16_mppi.hip", "f16_wind.hip", "f16_wind_ens.hip", "f16_observer.hip", "f16_debug.hip", "f16_tables.cpp"]
# the expression-exact (F16_STRICT) build of the plant alone: checker-side evidence that the device lookups and the plant
# reproduce the reference bit for bit where no libm call is involved (tests/test_gpu_dynamics.py); never used by the product
STRICT_SO_PATH = os.path.join(HERE, "libf16hip_strict.so")
STRICT_SOURCES = ["f16_api.hip", "f16_dynamics.hip", "f16_debug.hip", "f16_tables.cpp"]
# Default build: FMA contraction on, tan = sin/cos, tfac^4.14 = tfac^4 * exp(0.14 log tfac), branch-free sincos.  Held against
# multiprecision values by tests/test_gpu_elem.py: sin / cos within 1.3 ulp of the true value for |x| <= 1e6 (bound: libm's own error
# + 2 ulp), the reciprocal within 1 ulp, exp(0.14 log tfac) within 1 ulp (measured 0.64), qbar and ps within 9 and 10 x 2^-53 relative of
# their multiprecision values (measured 7.4 and 7.1; the density's share of that budget is 7 x 2^-53, up to 7 ulp of rho0 tfac^4.14),
# tan = sin * rcp(cos) within 13 x 2^-53.  Measured: xdot max rel. error vs the CPU restatement unchanged at
# 5e-14, -16 % kernel time.
# F16_STRICT=1 builds the expression-by-expression variant (no contraction, libm tan/pow): 97 % of xdot outputs
# then agree with the reference restatement bit for bit.
if os.environ.get("F16_STRICT"):
    _NUMERICS = ["-ffp-contract=off"]
else:
    _NUMERICS = ["-ffp-contract=fast", "-DF16_FAST_TAN", "-DF16_FAST_POW", "-DF16_FAST_TRIG", "-DF16_FAST_DIV"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result"] + _NUMERICS

_C = cabi.constants()                          # every value below is the header's `#define`
F16_ST = {k: _C["F16_ST_" + k] for k in ("ALPHA1", "ALPHA2", "BETA", "EL", "ENVELOPE", "NONFINITE", "QP_MAXITER", "QP_INFEASIBLE")}
F16_ST_ENV_STATE = lambda k: 1 << (8 + k)      # with ENVELOPE: state k was outside its box (env.py:117-124)
F16_ST_LOOP_STALL = _C["F16_ST_LOOP_STALL"]    # f16_rollout_mpc gave up waiting for the aircraft's previous step (a guard; never observed)
F16_ST_QP_SOFT_ACTIVE = _C["F16_ST_QP_SOFT_ACTIVE"]    # f16_mpc_plan_soft_rows: the returned solve has a soft state row outside its [l, u]
F16_FLAG_FIX_CLR = _C["F16_FLAG_FIX_CLR"]
F16_FLAG_NO_ENVELOPE = _C["F16_FLAG_NO_ENVELOPE"]
F16_FLAG_ONE_LANE = _C["F16_FLAG_ONE_LANE"]            # rollouts: the one-lane-per-aircraft kernel whatever the batch size (results independent of B)
F16_FLAG_HOLD_COMMAND = _C["F16_FLAG_HOLD_COMMAND"]    # closed MPC loops: a step without a command (infeasible QP, state not finite) keeps the previous one
F16_FLAG_NO_CELL_CACHE = _C["F16_FLAG_NO_CELL_CACHE"]  # diagnostic: quad rollout re-brackets every step (no cell re-use); results bit-identical either way
F16_INT_EULER, F16_INT_RK4 = _C["F16_INT_EULER"], _C["F16_INT_RK4"]    # the step rule of f16_rollout_rk / f16_rollout_lqr_rk / f16_rollout_cost_rk
INTEGRATORS = {"euler": F16_INT_EULER, "rk4": F16_INT_RK4}
F16_GS_ENTRIES = _C["F16_GS_ENTRIES"]          # doubles per node of a gain table: K[i][4 + j] at 3 i + j, the trim surface commands at 9 + i
F16_OBS_DOUBLES = _C["F16_OBS_DOUBLES"]        # doubles per observer model record: Ad[81] Bd[27] Lf[81] x9_trim[9] s_trim[3], padded (observer.py)


def integrator(method, rk4=True):
    """The `method` keyword of the rollouts ("euler" | "rk4") -> F16_INT_*; ValueError for anything else, and for "rk4" where the
    loop behind the call steps with the Euler step only (rk4=False)."""
    if not isinstance(method, str) or method not in INTEGRATORS:
        raise ValueError(f'method must be "euler" or "rk4", not {method!r}')
    if method == "rk4" and not rk4:
        raise ValueError('method="rk4" is not available here: this loop steps with the explicit Euler step')
    return INTEGRATORS[method]


class F16HipError(RuntimeError):
    pass


# The six structs of include/f16_hip.h: cabi.structure gives each class the header's fields and binds it to the C name, so that a
# parameter declared `const f16_wind *` is a POINTER(Wind).
@cabi.structure("f16_qp_settings")
class QPSettings(ctypes.Structure):
    """include/f16_hip.h `f16_qp_settings`: the ADMM settings of the MPC solves (f16_qp_default_settings fills in OSQP's defaults)."""


@cabi.structure("f16_mpc_weights")
class MPCWeights(ctypes.Structure):
    """include/f16_hip.h `f16_mpc_weights`: the arguments of utils.py:21 setup_OSQP / utils.py:219 dlqr that env.py fills with
    constants."""


@cabi.structure("f16_cost_weights")
class CostWeights(ctypes.Structure):
    """include/f16_hip.h `f16_cost_weights`: the diagonal weights of f16_rollout_cost (22 doubles, all finite and >= 0)."""


@cabi.structure("f16_gain_grid")
class GainGrid(ctypes.Structure):
    """include/f16_hip.h `f16_gain_grid`: the uniform (altitude, airspeed) grid of a gain schedule (nh, nv >= 2; dh, dv > 0)."""


@cabi.structure("f16_wind")
class Wind(ctypes.Structure):
    """include/f16_hip.h `f16_wind`: the air of f16_rollout_wind / f16_rollout_lqr_wind (device pointers; all NULL = still air)."""


@cabi.structure("f16_ens")
class Ens(ctypes.Structure):
    """include/f16_hip.h `f16_ens`: workspace, grouping and result arrays of the ensemble statistics (device pointers)."""


def make_cost_weights(q=None, qf=None, r=None, penalty=0.0):
    """CostWeights with the defaults q = qf = ones(9), r = ones(3): the diagonals of the reference's Q = Cd'Cd (Cd = I9) and R = I3."""
    import numpy as np
    w = CostWeights()
    for name, v, n in (("q", q, 9), ("qf", qf, 9), ("r", r, 3)):
        getattr(w, name)[:] = [1.0] * n if v is None else list(np.asarray(v, dtype=np.float64).reshape(n))
    w.pen = float(penalty)
    return w


def make_weights(Q=None, R=None, x_lb=None, x_ub=None, u_lb=None, u_ub=None, udot_lb=None, udot_ub=None):
    """MPCWeights from env.py's constants with the given entries replaced (None = all defaults -> None: the plain entry points)."""
    if all(v is None for v in (Q, R, x_lb, x_ub, u_lb, u_ub, udot_lb, udot_ub)):
        return None
    import numpy as np
    w = MPCWeights()
    load().f16_mpc_default_weights(ctypes.byref(w))
    if Q is not None:
        w.q_from_cd = 0
        w.Q[:] = list(np.asarray(Q, dtype=np.float64).reshape(81))
    if R is not None:
        w.R[:] = list(np.asarray(R, dtype=np.float64).reshape(9))
    for name, v, n in (("x_lb", x_lb, 9), ("x_ub", x_ub, 9), ("u_lb", u_lb, 3), ("u_ub", u_ub, 3), ("udot_lb", udot_lb, 3), ("udot_ub", udot_ub, 3)):
        if v is not None:
            getattr(w, name)[:] = list(np.asarray(v, dtype=np.float64).reshape(n))
    return w


def _fingerprint():
    """Hash of everything the binary depends on: every source / header under csrc/, the public header, the compiler
    flags (F16_STRICT, F16_HIPCC_EXTRA included).  Stored beside the .so at build time; load() refuses a stale binary."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h", ".hpp", ".inc")))
    for f in files + [os.path.join("..", "..", "include", "f16_hip.h")]:
        h.update(f.encode())
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(" ".join(HIPCC_FLAGS + os.environ.get("F16_HIPCC_EXTRA", "").split()).encode())
    return h.hexdigest()


def _compile_and_link(srcs, flags, out, verbose=False, stamp=None, fp=None, force=False):
    """One object per source, compiled in parallel and cached under build/obj/ by a hash of (source, every header, flags);
    then one link.  A change to one kernel file recompiles that file only.  One builder at a time per tree (file lock);
    the stamp is re-checked after the lock is taken and written inside it, so that the ranks of a multi-GPU run that all
    find a stale library do not relink in turn."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "..", "build", "obj")
    os.makedirs(objdir, exist_ok=True)
    import fcntl
    lock = open(os.path.join(objdir, ".lock"), "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    try:
        if not force and stamp and fp and os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == fp:
            return                      # another process built it while this one waited for the lock (force: relink regardless)
        _compile_and_link_locked(srcs, flags, out, verbose, hipcc, objdir)
        if stamp and fp:
            with open(stamp + ".tmp", "w") as f:
                f.write(fp + "\n")
            os.replace(stamp + ".tmp", stamp)
    finally:
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()


def _compile_and_link_locked(srcs, flags, out, verbose, hipcc, objdir):
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    hdr = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hpp", ".inc")):
            hdr.update(open(os.path.join(CSRC, f), "rb").read())
    hdr.update(open(os.path.join(HERE, "..", "include", "f16_hip.h"), "rb").read())
    cflags = [f for f in flags if f != "-shared"]
    hdr.update(" ".join(cflags).encode())

    def one(src):
        h = hashlib.sha256(hdr.digest() + open(src, "rb").read()).hexdigest()[:24]
        obj = os.path.join(objdir, os.path.basename(src) + "." + h + ".o")
        if not os.path.exists(obj):
            cmd = [hipcc] + cflags + ["-c", "-o", obj + ".tmp", src]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            os.replace(obj + ".tmp", obj)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 into the in-tree libf16hip.so (hipcc cross-compiles without a GPU).  Rebuilds
    when the recorded fingerprint (sources + flags) differs from the tree's."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    fp = _fingerprint()
    stamp = SO_PATH + ".stamp"
    if not force and os.path.exists(SO_PATH) and os.path.exists(stamp) and open(stamp).read().strip() == fp:
        return SO_PATH
    _compile_and_link(srcs, HIPCC_FLAGS + os.environ.get("F16_HIPCC_EXTRA", "").split(), SO_PATH, verbose, stamp, fp, force)
    return SO_PATH


def build_strict(force=False):
    """The F16_STRICT variant of the plant sources (no FMA contraction, IEEE divisions, libm tan/pow) as a second,
    test-only library."""
    import hashlib
    srcs = [os.path.join(CSRC, s) for s in STRICT_SOURCES]
    h = hashlib.sha256(_fingerprint().encode() + b"strict").hexdigest()
    stamp = STRICT_SO_PATH + ".stamp"
    if not force and os.path.exists(STRICT_SO_PATH) and os.path.exists(stamp) and open(stamp).read().strip() == h:
        return STRICT_SO_PATH
    flags = [f for f in HIPCC_FLAGS if f not in _NUMERICS] + ["-ffp-contract=off"]
    _compile_and_link(srcs, flags, STRICT_SO_PATH, False, stamp, h, force)
    return STRICT_SO_PATH


def strict_path():
    """Path of the up-to-date strict library, or an error naming the build command -- for callers that must not compile
    (GPU test processes: see load())."""
    import hashlib
    h = hashlib.sha256(_fingerprint().encode() + b"strict").hexdigest()
    stamp = STRICT_SO_PATH + ".stamp"
    if os.path.exists(STRICT_SO_PATH) and os.path.exists(stamp) and open(stamp).read().strip() == h:
        return STRICT_SO_PATH
    raise F16HipError(f"{STRICT_SO_PATH} is missing or stale: run `python -c 'import __graft_entry__ as g; g.build()'`")


_LIB = None


def load():
    """Load libf16hip.so once.  torch is imported first so that both share ONE HIP runtime
    (same libamdhip64 SONAME): device pointers from torch tensors are valid in our kernels."""
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  (must precede CDLL, see docstring)
    # load() never compiles: it may be called from a process that has already initialised the GPU (bench.run after
    # torch.cuda.set_device, or anything under `rocprofv3 -- python3 ...`, whose preload is inherited by children), and
    # the hipcc -> clang -> lld chain would be an exec hop of such a process.  A stale or missing binary is an error that
    # names the build command; F16_AUTOBUILD=1 opts back in for interactive use, and is ignored under a profiler preload.
    stamp = SO_PATH + ".stamp"
    build_cmd = "python -c 'import __graft_entry__ as g; g.build()'"
    stale = not os.path.exists(SO_PATH) or not os.path.exists(stamp) or open(stamp).read().strip() != _fingerprint()
    if stale and "F16HIP_SO" not in os.environ:
        profiled = bool(os.environ.get("LD_PRELOAD")) or any(k.startswith(("ROCP_", "ROCPROFILER_")) for k in os.environ)
        if os.environ.get("F16_AUTOBUILD") == "1" and not profiled:
            build()
        else:
            raise F16HipError(f"{SO_PATH} is missing or older than csrc/ (or built with other flags): run `{build_cmd}` "
                              f"first (load() does not compile; F16_AUTOBUILD=1 opts in outside a profiler)")
    if not os.path.exists(SO_PATH):
        raise F16HipError(f"{SO_PATH} is missing: run `{build_cmd}`")
    L = ctypes.CDLL(SO_PATH)
    cabi.declare(L)      # every signature include/f16_hip.h declares; a symbol an older or plant-only library lacks is skipped
    _LIB = L
    return L


def check(rc, L=None):
    if rc != 0:
        L = L or load()
        raise F16HipError(f"libf16hip error {rc}: {L.f16_last_error().decode()}")


class Context:
    """Owns one f16_ctx (device table image) on one GPU."""

    def __init__(self, device=0):
        self.lib = load()
        self.handle = ctypes.c_void_p()
        check(self.lib.f16_create(ctypes.byref(self.handle), int(device)), self.lib)
        self.device = int(device)

    def close(self):
        if self.handle:
            self.lib.f16_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
