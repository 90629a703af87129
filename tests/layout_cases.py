"""The leading-dimension contract of include/f16_hip.h -- "element k of aircraft b lives at p[k*ld + b], ld >= B" -- as ONE table
(ROWS: every array argument of every batched entry point this module holds to it) and the harness that checks a row: the same
host inputs go through a TIGHT call (ld = B, arrays allocated exactly) and a PADDED call (odd ld >= B + 3, every array a view into
a larger allocation, one element past a 16-byte boundary, guards before and behind, sentinels in guards, outputs and padding), and
`compare` holds the padded call to the tight one bit for bit.  Pure numpy here: tests/test_cabi_layout_cpu.py checks the table
against the header and the harness against numpy stand-ins for a wrong kernel; tests/test_gpu_cabi_layout.py runs CASES on the
device.  What the tight call's numbers are worth is pinned elsewhere in the suite; nothing here asserts accuracy."""
import ctypes

import numpy as np

FOREIGN = 1 << 30                      # a status bit no kernel sets (tests/test_gpu_trim_lockstep.py): sticky entries must keep it
SENT_I32 = -7                          # int32 sentinel: guards, outputs, padding columns
SENT_F64 = 0x7FF800005EA7BEEF          # fp64 sentinel: a quiet NaN with a payload of its own, written and compared as int64
NAN_F64 = int(np.array(np.nan).view(np.int64))      # the plain NaN in the padding columns of fp64 inputs
GUARD = 64                             # guard elements before the first and behind the last row (at least)
OFFSET = 65                            # elements in front of a padded view: >= GUARD and one element past a 16-byte boundary


def padded_ld(B):
    """the first odd number >= B + 3"""
    return B + 3 if (B + 3) % 2 else B + 4


# ------------------------------------------------------------------------------------------------ the table
class Arg:
    """One array argument: header name; rows in front of [ld] (an int or a function of the case's sizes); dtype "f8" | "i4"; its
    leading dimension "ld" | "ld0" | None (a flat array without a batch axis: `rows` elements); role "in" | "out" | "inout";
    optional = the header says "may be NULL"."""

    def __init__(self, name, rows, role="in", ld="ld", dtype="f8", optional=False):
        assert role in ("in", "out", "inout") and ld in ("ld", "ld0", None) and dtype in ("f8", "i4")
        self.name, self._rows, self.role, self.ld, self.dtype, self.optional = name, rows, role, ld, dtype, optional

    def rows(self, n):
        return int(self._rows(n) if callable(self._rows) else self._rows)


class Row:
    """One entry point: its array arguments and its status rule -- "sticky" (read, OR-ed into, written back: a bit that is set
    survives), "output" (every word overwritten from 0), "read" (only read) or None (no status argument)."""

    def __init__(self, *args, status=None):
        assert status in ("sticky", "output", "read", None)
        self.args, self.status = list(args), status
        assert (status is None) == ("status" not in [a.name for a in args])


def I(name, rows, **kw):
    return Arg(name, rows, "in", **kw)


def O(name, rows, **kw):
    return Arg(name, rows, "out", **kw)


def IO(name, rows, **kw):
    return Arg(name, rows, "inout", **kw)


def ST(rows=1, ld="ld", optional=True):
    """a sticky status column (or `rows` slices of one)"""
    return Arg("status", rows, "inout", ld=ld, dtype="i4", optional=optional)


S = lambda n: -(-n["nsteps"] // n["hold"])                          # rows of a schedule
SAMPLES = lambda n: n["nsteps"] // n["traj_every"]                  # stored samples of a plant rollout
TRAJ = O("traj", lambda n: SAMPLES(n) * 18, optional=True)
NH = lambda n: n["hzn_hi"] - n["hzn_lo"] + 1
NCTRL = lambda n: n["nctrl"]
LOOP_TRAJ = O("traj", lambda n: n["nctrl"] * n["hold"] // n["traj_every"] * 18, optional=True)
MODEL_TRAJ = O("model_traj", lambda n: n["nctrl"] // n["model_every"] * 189, optional=True)
DEM_ROWS = lambda n: -(-n["nctrl"] // n["dem_hold"]) * 3
MODEL = (I("Ad", 81), I("Bd", 27), I("Cd", 81))
QP_OUT = (O("u_cmd", 3), O("u_seq", lambda n: 3 * n["hzn"], optional=True), O("info", 4, optional=True))
LOOP_OUT = (O("cmd_traj", lambda n: NCTRL(n) * 3, optional=True), O("iters_traj", NCTRL, dtype="i4", optional=True))
RELIN = (IO("x", 18), IO("u", 4))
RELIN_OUT = (O("traj", lambda n: SAMPLES(n) * 18, optional=True), O("u_traj", lambda n: SAMPLES(n) * 3, optional=True),
             O("K_traj", lambda n: SAMPLES(n) * 27, optional=True))
COST = (I("x0", 18, ld="ld0"), I("u_seq", lambda n: S(n) * 4), I("x_ref", 9, ld="ld0"), I("u_ref", 3, ld="ld0", optional=True),
        O("cost", 1), O("x_end", 18, optional=True), TRAJ, Arg("status", 1, "out", dtype="i4", optional=True))

ROWS = {
    # plant evaluations
    "f16_xdot_batch": Row(I("x", 18), I("u", 4), O("xdot", 18), ST(), status="sticky"),
    "f16_nlplant_batch": Row(I("xu", 18), O("xdot", 18), ST(), status="sticky"),
    "f16_xdot_na_batch": Row(I("x_full", 18), I("x9", 9), I("u3", 3), O("xdot9", 9), ST(), status="sticky"),
    # plant rollouts
    "f16_rollout": Row(IO("x", 18), I("u", 4), TRAJ, ST(), status="sticky"),
    "f16_rollout_lqr": Row(IO("x", 18), I("u0", 4), I("K", 27), I("dem", 3), TRAJ, O("u_out", 4, optional=True), ST(), status="sticky"),
    "f16_rollout_lqr_sched": Row(IO("x", 18), I("u0", 4), I("K", 27), I("dem_seq", lambda n: S(n) * 3), TRAJ, O("u_out", 4, optional=True),
                                 ST(), status="sticky"),
    "f16_rollout_rk": Row(IO("x", 18), I("u_seq", lambda n: S(n) * 4), TRAJ, ST(), status="sticky"),
    "f16_rollout_lqr_rk": Row(IO("x", 18), I("u0", 4), I("K", 27), I("dem_seq", lambda n: S(n) * 3), TRAJ, O("u_out", 4, optional=True),
                              ST(), status="sticky"),
    "f16_rollout_cost_rk": Row(*COST, status="output"),
    "f16_rollout_lqr_gs": Row(IO("x", 18), I("u0", 4), I("tab", lambda n: n["nh"] * n["nv"] * 12, ld=None), I("dem_seq", lambda n: S(n) * 3),
                              TRAJ, O("u_out", 4, optional=True), O("gs_out", 1, dtype="i4", optional=True), ST(), status="sticky"),
    "f16_rollout_lqr_linear": Row(IO("x9", 9), I("Ad", 81), I("Bd", 27), I("K", 27), I("x_ref", 9), I("u0", 3, optional=True),
                                  O("traj_x", lambda n: SAMPLES(n) * 9, optional=True), O("traj_u", lambda n: SAMPLES(n) * 3, optional=True)),
    # control chain
    "f16_linearise_batch": Row(I("x", 18), I("u", 4), O("Ac", 81), O("Bc", 27), O("Cc", 81), ST(optional=False), status="sticky"),
    "f16_linearise_full_batch": Row(I("x", 18), I("u", 4), O("Ac", 324), O("Bc", 72), O("Cc", 180), ST(optional=False), status="sticky"),
    "f16_c2d_batch": Row(I("Ac", 81), I("Bc", 27), O("Ad", 81), O("Bd", 27)),
    "f16_c2d_full_batch": Row(I("Ac", 324), I("Bc", 72), O("Ad", 324), O("Bd", 72)),
    "f16_lqr_batch": Row(*MODEL, O("K", 27), O("Pare", 81, optional=True), ST(), status="sticky"),
    "f16_lqr_batch_w": Row(*MODEL, O("K", 27), O("Pare", 81, optional=True), ST(), status="sticky"),
    "f16_rollout_lqr_relin": Row(*RELIN, I("x_ref", 9), I("u0", 3, optional=True), *RELIN_OUT, ST(), status="sticky"),
    "f16_rollout_lqr_relin_sched": Row(*RELIN, I("xref_seq", lambda n: S(n) * 9), I("u0", 3, optional=True), *RELIN_OUT, ST(), status="sticky"),
    # MPC: one-shot solves, the horizon sweep, plans (arrays at the ld the plan was created with), the QP alone
    "f16_mpc_batch": Row(*MODEL, I("x", 18), I("dem", 3), *QP_OUT, ST(), status="sticky"),
    "f16_mpc_batch_w": Row(*MODEL, I("x", 18), I("dem", 3), I("x_ref", 9, optional=True), *QP_OUT, ST(), status="sticky"),
    "f16_mpc_hzn_sweep": Row(*MODEL, I("x", 18), I("dem", 3), O("u_cmd", lambda n: NH(n) * 3), O("info", lambda n: NH(n) * 4, optional=True),
                             ST(NH), status="sticky"),
    "f16_mpc_plan_create": Row(*MODEL),
    "f16_mpc_plan_create_w": Row(*MODEL),
    "f16_mpc_plan_solve": Row(I("x", 18), I("dem", 3), *QP_OUT, ST(), status="sticky"),
    "f16_mpc_plan_solve_w": Row(I("x", 18), I("dem", 3), I("x_ref", 9, optional=True), *QP_OUT, ST(), status="sticky"),
    "f16_mpc_qp_debug": Row(*MODEL, I("x", 18), I("dem", 3)),
    "f16_mpc_qp_debug_w": Row(*MODEL, I("x", 18), I("dem", 3), I("x_ref", 9, optional=True)),
    # closed MPC loops on a plan
    "f16_rollout_mpc": Row(*RELIN, I("dem", 3), LOOP_TRAJ, *LOOP_OUT, ST(), status="sticky"),
    "f16_rollout_mpc_hold": Row(*RELIN, I("dem", 3), LOOP_TRAJ, *LOOP_OUT, ST(), status="sticky"),
    "f16_rollout_mpc_sched": Row(*RELIN, I("dem_seq", DEM_ROWS), LOOP_TRAJ, *LOOP_OUT, ST(), status="sticky"),
    "f16_rollout_mpc_relin_hold": Row(*RELIN, I("dem", 3), LOOP_TRAJ, *LOOP_OUT, MODEL_TRAJ, ST(), status="sticky"),
    "f16_rollout_mpc_relin_sched": Row(*RELIN, I("dem_seq", DEM_ROWS), LOOP_TRAJ, *LOOP_OUT, MODEL_TRAJ, ST(), status="sticky"),
}

# Entry points whose padded case lives in another module: symbol -> (test file, test function).  Each named test drives the symbol
# with ld > B (ld = B + 3, B + 5 or B + 37), NaN or a sentinel in the padding, and checks that the padding comes back untouched.
COVERED_ELSEWHERE = {
    "f16_rollout_sched": ("tests/test_gpu_rollout_sched.py", "test_degenerate_schedules"),
    "f16_rollout_cost": ("tests/test_gpu_rollout_cost.py", "test_cost_equals_its_definition"),
    "f16_mppi_blend": ("tests/test_gpu_rollout_cost.py", "test_blend_against_the_reference_rule"),
    "f16_mppi_sample": ("tests/test_gpu_mppi_loop.py", "test_sampler_against_the_reference"),
    "f16_rollout_mppi": ("tests/test_gpu_mppi_loop.py", "test_fused_equals_the_host_loop_bit_for_bit"),
    "f16_xdot_wind_batch": ("tests/test_gpu_wind.py", "test_xdot_against_the_twin"),
    "f16_rollout_wind": ("tests/test_gpu_wind.py", "test_rollouts_against_the_twin"),
    "f16_rollout_lqr_wind": ("tests/test_gpu_wind.py", "test_rollouts_against_the_twin"),
    "f16_gust_sample": ("tests/test_gpu_wind.py", "test_gust_sample_against_the_reference"),
    "f16_rollout_wind_ens": ("tests/test_gpu_ensemble.py", "test_statistics_equal_the_reference_of_the_same_samples"),
    "f16_rollout_lqr_wind_ens": ("tests/test_gpu_ensemble.py", "test_statistics_equal_the_reference_of_the_same_samples"),
    "f16_ens_from_traj": ("tests/test_gpu_ensemble.py", "test_statistics_equal_the_reference_of_the_same_samples"),
    "f16_kalman_batch": ("tests/test_gpu_lqg.py", "test_kalman_batch_against_scipy"),
    "f16_observer_step": ("tests/test_gpu_lqg.py", "test_observer_step_against_the_reference"),
    "f16_rollout_lqg_wind": ("tests/test_gpu_lqg.py", "test_split_calls_continue_one_flight"),
    "f16_rollout_lqg_wind_ens": ("tests/test_gpu_lqg.py", "test_ensemble_twin"),
    "f16_trim_batch": ("tests/test_gpu_trim_lockstep.py", "test_lockstep_with_scipy"),
    "f16_trim_man_batch": ("tests/test_gpu_trim_man.py", "test_lockstep_with_scipy"),
    "f16_rollout_mpc_relin": ("tests/test_gpu_mpc_relin.py", "test_relin_loop_column_of_a_padded_batch_equals_a_batch_of_one"),
}


def contract_symbols(functions):
    """the functions of cabi.functions() (or of cabi.parse(text)[0]) the contract applies to: a parameter named ld or ld0, or a
    f16_mpc_plan * together with a device array (a pointer that is not ctx / stream / plan / h_* / a pointer to a struct)"""
    out = []
    for name, (_, params) in functions.items():
        names = [p for _, p in params]
        if "ld" in names or "ld0" in names or ("plan" in names and array_parameters(params)):
            out.append(name)
    return out


def array_parameters(params):
    """the parameter names a row has to list: every pointer but ctx, stream, plan, h_* and pointers to structs (a struct pointer is a
    ctypes POINTER(Structure) after cabi.functions(), the struct's name before)"""
    out = []
    for t, p in params:
        pointer = t is ctypes.c_void_p or isinstance(t, str) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))
        struct = isinstance(t, str) or (isinstance(t, type) and issubclass(t, ctypes._Pointer) and issubclass(t._type_, ctypes.Structure))
        if pointer and not struct and p not in ("ctx", "stream", "plan") and not p.startswith("h_"):
            out.append(p)
    return out


# ------------------------------------------------------------------------------------------------ the harness
class Buf:
    """One array of one call on the host, as raw bits (int64 for fp64, int32): `full` is the allocation that is uploaded, `view`
    [rows, ld] the argument inside it (a flat array: [1, rows]), `before` a copy taken before the call, `after` what came back."""

    def __init__(self, arg, n, B, ld, padded, data=None, sticky=False, null=False):
        self.arg, self.padded, self.null = arg, padded, null
        self.rows, self.B, self.ld = (arg.rows(n), B, ld) if arg.ld else (1, arg.rows(n), arg.rows(n))
        self.f8 = arg.dtype == "f8"
        self.sent = SENT_F64 if self.f8 else SENT_I32
        self.off = OFFSET if padded else 0
        size = self.rows * self.ld
        self.full = np.full(self.off + size + (GUARD if padded else 0), self.sent, dtype=np.int64 if self.f8 else np.int32)
        v = self.view(self.full)
        if arg.role != "out":
            v[:, self.B:] = NAN_F64 if self.f8 else SENT_I32
            if sticky:
                v[:, :self.B] = FOREIGN if padded else 0
            else:
                d = np.ascontiguousarray(data, dtype=np.float64 if self.f8 else np.int32).reshape(self.rows, self.B)
                v[:, :self.B] = d.view(self.full.dtype)
        self.before, self.after = self.full.copy(), None

    def view(self, full):
        return full[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)

    @property
    def itemsize(self):
        return self.full.dtype.itemsize


def layout(args, n, B, B0, padded, data, status_rule, null_optional_outputs=False):
    """the arrays of one call: {name: Buf}.  data: {name: [rows, B] host array} for every input and in/out array but a sticky status"""
    ld, ld0 = (padded_ld(B), padded_ld(B0)) if padded else (B, B0)
    bufs = {}
    for a in args:
        sticky = a.name == "status" and status_rule == "sticky"
        null = null_optional_outputs and a.optional and a.role != "in"
        bufs[a.name] = Buf(a, n, B0 if a.ld == "ld0" else B, ld0 if a.ld == "ld0" else ld, padded, None if sticky else data.get(a.name), sticky, null)
    return bufs, ld, ld0


def _first(mask):
    r, c = np.argwhere(mask)[0]
    return f"first at slice {r}, column {c}, {int(mask.sum())} element(s)"


def compare(args, status_rule, tight, padded):
    """What the contract asks of a padded call against the tight call of the same inputs, all bitwise -> the list of violations
    (empty: the row holds).  tight / padded: {name: Buf} with `after` filled in."""
    bad = []
    for a in args:
        t, p = tight[a.name], padded[a.name]
        if t.null or p.null:
            continue
        tv, pb, pa = t.view(t.after), p.view(p.before), p.view(p.after)
        B = p.B
        if a.name == "status" and status_rule == "sticky":
            tw, pw = tv[:, :B], pa[:, :B]
            if (tw & FOREIGN).any():
                bad.append(f"status: the tight call, started from 0, carries FOREIGN ({_first((tw & FOREIGN) != 0)})")
            if ((pw & FOREIGN) == 0).any():
                bad.append(f"status: a foreign bit that was set did not survive the call ({_first((pw & FOREIGN) == 0)})")
            if ((pw & (FOREIGN - 1)) != (tw & (FOREIGN - 1))).any():
                bad.append(f"status: bits below FOREIGN differ from the tight call ({_first((pw & (FOREIGN - 1)) != (tw & (FOREIGN - 1)))})")
            if (pw != (tw | FOREIGN)).any():
                bad.append(f"status: padded != tight | FOREIGN ({_first(pw != (tw | FOREIGN))})")
        elif a.role != "in":
            if (pa[:, :B] != tv[:, :B]).any():
                bad.append(f"{a.name}: columns < B differ from the tight call ({_first(pa[:, :B] != tv[:, :B])})")
        elif (pa[:, :B] != pb[:, :B]).any():
            bad.append(f"{a.name}: an input was written ({_first(pa[:, :B] != pb[:, :B])})")
        if (pa[:, B:] != pb[:, B:]).any():
            bad.append(f"{a.name}: padding columns B .. ld-1 were written ({_first(pa[:, B:] != pb[:, B:])})")
        front, back = p.after[:p.off], p.after[p.off + p.rows * p.ld:]
        if (front != p.sent).any() or (back != p.sent).any():
            where = "before" if (front != p.sent).any() else "behind"
            bad.append(f"{a.name}: a guard element {where} the array was written")
        if t.after.shape != t.before.shape or (a.role == "in" and (t.after != t.before).any()):
            bad.append(f"{a.name}: the tight call wrote an input")
    return bad


def compare_required(args, padded, bare):
    """the padded call with every optional output NULL against the padded call: the required outputs, bit for bit, guards and
    padding included"""
    bad = []
    for a in args:
        if a.role != "in" and not bare[a.name].null and (padded[a.name].after != bare[a.name].after).any():
            bad.append(f"{a.name}: differs when the optional outputs are NULL ({int((padded[a.name].after != bare[a.name].after).sum())} element(s))")
    return bad


# ------------------------------------------------------------------------------------------------ the cases
EULER, RK4 = 1, 4                      # F16_INT_EULER, F16_INT_RK4 (checked against the header by the CPU module)
ONE_LANE = 4                           # F16_FLAG_ONE_LANE
DT, EPS = 0.001, 1e-5
DEM = (0.02, -0.01, 0.01)              # the MPC demands of every case
SOFT = (0.0, 0.0, 100.0, 100.0, 100.0, 100.0, 100.0, 0.0, 100.0)       # soft rows at weight 100 on the six bounded state rows


class Case:
    """id; the symbols whose rows supply the arrays; the sizes the rows' functions read (B, B0 and whatever else); data(src, n) ->
    {name: [rows, B] host array}; run(api): the calls.  src is the GPU module's provider of states, models and gains."""

    def __init__(self, id, symbols, n, data, run):
        self.id, self.symbols, self.n, self.data, self.run = id, symbols, dict(n), data, run
        self.n.setdefault("B0", self.n["B"])

    def args(self):
        seen = {}
        for s in self.symbols:
            for a in ROWS[s].args:
                seen.setdefault(a.name, a)
        return list(seen.values())

    def status_rule(self):
        rules = {ROWS[s].status for s in self.symbols} - {None}
        assert len(rules) <= 1
        return rules.pop() if rules else None


def one(symbol, **scalars):
    """a case that is one call"""
    return lambda api: api.call(symbol, **scalars)


def _rows(base, Srows, scale):
    """[rows, B] -> [Srows * rows, B]: schedule row s is base * (1 + scale * s)"""
    return np.concatenate([base * (1.0 + scale * s) for s in range(Srows)])


def plant_data(fi, xcg=0.25):
    def data(src, n):
        x, u = src.states(n["B"])
        x9 = x[src.mpc_x_idx] * 1.01
        return dict(x=x, u=u, xu=np.concatenate([x[:12], u, x[16:18]]), x_full=x, x9=x9, u3=u[1:4] * 0.9)
    return data


def rollout_data(src, n):
    B = n["B"]
    x, u = src.states(B)
    K, dem = src.gain(B)
    d = dict(x=x, u=u, u0=u, K=K, dem=dem)
    if "hold" in n:
        d.update(u_seq=_rows(u, S(n), 0.01), dem_seq=_rows(dem, S(n), -0.5))
    if "nh" in n:
        d["tab"] = np.random.default_rng(5).uniform(-0.5, 0.5, n["nh"] * n["nv"] * 12)
    return d


def cost_data(src, n):
    B, B0 = n["B"], n["B0"]
    x, u = src.states(B0)
    lanes = np.arange(B)
    ul = u[:, lanes % B0] * (1.0 + 0.002 * (lanes // B0))[None]
    return dict(x0=x, u_seq=_rows(ul, S(n), 0.01), x_ref=x[src.mpc_x_idx], u_ref=u[1:4] * 0.5)


def chain_data(src, n):
    m = src.model(n["B"], "chain")
    return dict(x=m["x"], u=m["u"], Ac=m["Ac"], Bc=m["Bc"], Ad=m["Ad"], Bd=m["Bd"], Cd=m["Cd"])


def chain_full_data(src, n):
    m = src.model(n["B"], "chain")
    return dict(x=m["x"], u=m["u"], Ac=m["Ac18"], Bc=m["Bc18"])


def linear_data(src, n):
    m = src.model(n["B"], "chain")
    x9 = m["x"][src.mpc_x_idx]
    xr = x9.copy()
    xr[4:7] = np.array(DEM)[:, None]
    return dict(x9=x9, Ad=m["Ad"], Bd=m["Bd"], K=m["K"], x_ref=xr, u0=m["u"][1:4])


def relin_data(src, n):
    m = src.model(n["B"], "mpc")
    x9 = m["x"][src.mpc_x_idx]
    xr = x9.copy()
    xr[4:7] = np.array(DEM)[:, None]
    return dict(x=m["x"], u=m["u"], x_ref=xr, xref_seq=_rows(xr, S(n) if "hold" in n else 1, 0.01), u0=m["u"][1:4])


def mpc_data(kind="mpc"):
    def data(src, n):
        m = src.model(n["B"], kind)
        dem = np.tile(np.array(DEM)[:, None], (1, n["B"]))
        xr = m["x"][src.mpc_x_idx].copy()
        xr[4:7] = dem
        d = dict(Ad=m["Ad"], Bd=m["Bd"], Cd=m["Cd"], x=m["x"], u=m["u"], dem=dem, x_ref=xr)
        if "dem_hold" in n:
            d["dem_seq"] = _rows(dem, DEM_ROWS(n) // 3, -0.5)
        return d
    return data


def mpc_run(symbol, hzn, **settings):
    return lambda api: api.call(symbol, hzn=hzn, dt=DT, s=api.settings(**settings))


def plan_run(create, solve, hzn, warm=False, soft=False):
    def run(api):
        with api.plan(create, hzn, DT) as plan:
            if soft:
                api.soft_rows(plan, SOFT)
            if warm:
                api.warm_start(plan)
                api.call(solve, plan=plan)
            api.call(solve, plan=plan)
    return run


def loop_run(symbol, plan_dt, **scalars):
    def run(api):
        with api.plan("f16_mpc_plan_create_w", 10, plan_dt) as plan:
            api.call(symbol, plan=plan, xcg=0.35, fi_flag=1, flags=0, **scalars)
    return run


def qp_run(symbol):
    """the QP of aircraft 2 at hzn = 3 on the host: n = 9 unknowns, 45 rows"""
    def run(api):
        extra = dict(h_w=api.weights()) if symbol.endswith("_w") else {}
        api.call(symbol, b=2, hzn=3, dt=DT, h_P=api.host("h_P", 81), h_q=api.host("h_q", 9), h_A=api.host("h_A", 45 * 9), h_l=api.host("h_l", 45),
                 h_u=api.host("h_u", 45), **extra)
    return run


def _cases():
    c = []
    plant = dict(xcg=0.25, flags=0)
    # plant evaluations: a short second wave, and beyond the 256-aircraft branch of f16_nlplant_batch
    for sym in ("f16_xdot_batch", "f16_nlplant_batch", "f16_xdot_na_batch"):
        for B in (65, 300):
            for fi in (1, 0):
                c.append(Case(f"{sym}-B{B}-fi{fi}", [sym], dict(B=B), plant_data(fi), one(sym, fi_flag=fi, **plant)))
    # Euler rollouts: 34 steps (past the 32-step re-evaluation of the carried sin / cos pairs), samples at 17 and 34; one B per
    # kernel of rollout_dispatch: quad<1> (a ragged group), quad<2>, 4-wave, 128 / 256 lanes, 512 lanes on the integer image
    euler = [(B, 1, 0) for B in (19, 4100, 8200, 16400, 33000, 131100)] + [(B, 0, 0) for B in (19, 16400, 131100)] + [(65, 1, ONE_LANE), (65, 0, ONE_LANE)]
    for sym in ("f16_rollout", "f16_rollout_lqr"):
        for B, fi, flags in euler:
            c.append(Case(f"{sym}-B{B}-fi{fi}-flags{flags}", [sym], dict(B=B, nsteps=34, traj_every=17), rollout_data,
                          one(sym, nsteps=34, traj_every=17, dt=DT, xcg=0.25, fi_flag=fi, flags=flags)))
    # (f16_rollout_lqr_sched has no padded case elsewhere: the quad, 4-wave and 256-lane twins)
    for B in (19, 8200, 33000):
        n = dict(B=B, nsteps=34, hold=16, traj_every=17)
        c.append(Case(f"f16_rollout_lqr_sched-B{B}", ["f16_rollout_lqr_sched"], n, rollout_data,
                      one("f16_rollout_lqr_sched", nsteps=34, hold=16, traj_every=17, dt=DT, xcg=0.25, fi_flag=1, flags=0)))
    # the step rule as an argument: 64 lanes, 256 lanes, and 256 lanes in a second pass over the grid (RK4 never runs 512)
    rk = dict(nsteps=6, hold=3, traj_every=3)
    for sym in ("f16_rollout_rk", "f16_rollout_lqr_rk"):
        for method in (EULER, RK4):
            for B, fi in ((65, 1), (33000, 1), (131100, 1), (65, 0)):
                c.append(Case(f"{sym}-m{method}-B{B}-fi{fi}", [sym], dict(B=B, **rk), rollout_data,
                              one(sym, dt=DT, xcg=0.25, fi_flag=fi, method=method, flags=0, **rk)))
    for B0, K, method in ((5, 13, EULER), (5, 13, RK4), (300, 110, RK4)):
        c.append(Case(f"f16_rollout_cost_rk-m{method}-B0{B0}-K{K}", ["f16_rollout_cost_rk"], dict(B=B0 * K, B0=B0, **rk), cost_data,
                      lambda api, method=method: api.call("f16_rollout_cost_rk", h_w=api.cost_weights(), dt=DT, xcg=0.25, fi_flag=1, method=method,
                                                          flags=0, **rk)))
    for B, method in ((65, EULER), (65, RK4), (33000, RK4), (131100, EULER)):
        n = dict(B=B, nh=2, nv=2, **rk)
        c.append(Case(f"f16_rollout_lqr_gs-m{method}-B{B}", ["f16_rollout_lqr_gs"], n, rollout_data,
                      lambda api, method=method: api.call("f16_rollout_lqr_gs", h_grid=api.gain_grid(5000.0, 25000.0, 400.0, 450.0, 2, 2), gs_every=2,
                                                          dt=DT, xcg=0.25, fi_flag=1, method=method, flags=0, **rk)))
    c.append(Case("f16_rollout_lqr_linear-B70", ["f16_rollout_lqr_linear"], dict(B=70, nsteps=5, traj_every=1), linear_data,
                  one("f16_rollout_lqr_linear", nsteps=5, traj_every=1, track_mask=0x70)))
    # control chain
    for B in (5, 70):
        c.append(Case(f"f16_linearise_batch-B{B}", ["f16_linearise_batch"], dict(B=B), chain_data,
                      one("f16_linearise_batch", eps=EPS, xcg=0.25, fi_flag=1, flags=0)))
        c.append(Case(f"f16_linearise_full_batch-B{B}", ["f16_linearise_full_batch"], dict(B=B), chain_full_data,
                      one("f16_linearise_full_batch", eps=EPS, xcg=0.25, fi_flag=1, flags=0)))
        c.append(Case(f"f16_c2d_batch-B{B}", ["f16_c2d_batch"], dict(B=B), chain_data, one("f16_c2d_batch", dt=DT)))
        c.append(Case(f"f16_c2d_full_batch-B{B}", ["f16_c2d_full_batch"], dict(B=B), chain_full_data, one("f16_c2d_full_batch", dt=DT)))
        c.append(Case(f"f16_lqr_batch-B{B}", ["f16_lqr_batch"], dict(B=B), chain_data, one("f16_lqr_batch")))
        c.append(Case(f"f16_lqr_batch_w-B{B}", ["f16_lqr_batch_w"], dict(B=B), chain_data,
                      lambda api: api.call("f16_lqr_batch_w", h_w=api.weights())))
    # one-shot MPC: OSQP's defaults -- hzn 10, 30 the wavefront solver, 32 the 512-lane solver, 33, 41 k_mpc_big (inside and beyond
    # the plan limit); the builder's settings -- hzn 2, 10, 32 the three k_mpc_fast instantiations; a negative max_iter: the generic
    # kernel.  B = 20 for hzn <= 32 (above the 16-aircraft threshold of the wavefront solver's spreading), B = 3 beyond.
    solves = [(h, {}) for h in (10, 30, 32, 33, 41)] + [(h, dict(scaling=0, rho=0.0)) for h in (2, 10, 32)] + [(10, dict(max_iter=-40000))]
    for sym in ("f16_mpc_batch", "f16_mpc_batch_w"):
        for hzn, st in solves:
            tag = "-".join(f"{k}{v}" for k, v in st.items()) or "osqp"
            run = mpc_run(sym, hzn, **st) if sym == "f16_mpc_batch" else \
                (lambda api, hzn=hzn, st=st: api.call("f16_mpc_batch_w", h_w=api.weights(), hzn=hzn, dt=DT, s=api.settings(**st)))
            c.append(Case(f"{sym}-hzn{hzn}-{tag}", [sym], dict(B=20 if hzn <= 32 else 3, hzn=hzn), mpc_data(), run))
    c.append(Case("f16_mpc_hzn_sweep-31-35", ["f16_mpc_hzn_sweep"], dict(B=3, hzn_lo=31, hzn_hi=35), mpc_data(),
                  lambda api: api.call("f16_mpc_hzn_sweep", hzn_lo=31, hzn_hi=35, dt=DT, s=api.settings())))
    for create, solve, hzn, B, kw in (("f16_mpc_plan_create_w", "f16_mpc_plan_solve_w", 10, 20, {}),
                                      ("f16_mpc_plan_create_w", "f16_mpc_plan_solve_w", 10, 20, dict(warm=True)),
                                      ("f16_mpc_plan_create_w", "f16_mpc_plan_solve_w", 10, 20, dict(soft=True)),
                                      ("f16_mpc_plan_create_w", "f16_mpc_plan_solve_w", 30, 20, {}),
                                      ("f16_mpc_plan_create", "f16_mpc_plan_solve", 30, 20, dict(warm=True)),
                                      ("f16_mpc_plan_create_w", "f16_mpc_plan_solve_w", 33, 3, {}),
                                      ("f16_mpc_plan_create", "f16_mpc_plan_solve", 33, 3, {})):
        c.append(Case(f"{solve}-hzn{hzn}" + "".join("-" + k for k in kw), [create, solve], dict(B=B, hzn=hzn), mpc_data(),
                      plan_run(create, solve, hzn, **kw)))
    for sym in ("f16_mpc_qp_debug", "f16_mpc_qp_debug_w"):
        c.append(Case(f"{sym}-B5", [sym], dict(B=5, hzn=3), mpc_data(), qp_run(sym)))
    # closed MPC loops: B = 20, hzn = 10, four control steps
    loop = dict(B=20, hzn=10, nctrl=4, hold=1, traj_every=1, model_every=1, dem_hold=1)
    cw = "f16_mpc_plan_create_w"
    c.append(Case("f16_rollout_mpc", [cw, "f16_rollout_mpc"], loop, mpc_data(), loop_run("f16_rollout_mpc", DT, nsteps=4, traj_every=1)))
    c.append(Case("f16_rollout_mpc_hold", [cw, "f16_rollout_mpc_hold"], dict(loop, hold=3, traj_every=3), mpc_data("mpc3"),
                  loop_run("f16_rollout_mpc_hold", 3 * DT, nctrl=4, hold=3, traj_every=3, dt=DT)))
    c.append(Case("f16_rollout_mpc_sched", [cw, "f16_rollout_mpc_sched"], dict(loop, dem_hold=2), mpc_data(),
                  loop_run("f16_rollout_mpc_sched", DT, nctrl=4, hold=1, dem_hold=2, traj_every=1, dt=DT)))
    c.append(Case("f16_rollout_mpc_relin_hold", [cw, "f16_rollout_mpc_relin_hold"], dict(loop, hold=3, traj_every=3, model_every=2), mpc_data("mpc3"),
                  loop_run("f16_rollout_mpc_relin_hold", 3 * DT, nctrl=4, hold=3, traj_every=3, model_every=2, dt=DT, eps=EPS)))
    c.append(Case("f16_rollout_mpc_relin_sched", [cw, "f16_rollout_mpc_relin_sched"], dict(loop, dem_hold=2), mpc_data(),
                  loop_run("f16_rollout_mpc_relin_sched", DT, nctrl=4, hold=1, dem_hold=2, traj_every=1, model_every=1, dt=DT, eps=EPS)))
    relin = dict(nsteps=4, traj_every=1, track_mask=0x70, eps=EPS, dt=DT, xcg=0.35, fi_flag=1, flags=0)
    c.append(Case("f16_rollout_lqr_relin", ["f16_rollout_lqr_relin"], dict(B=20, nsteps=4, traj_every=1), relin_data,
                  lambda api: api.call("f16_rollout_lqr_relin", h_w=None, **relin)))
    c.append(Case("f16_rollout_lqr_relin_sched", ["f16_rollout_lqr_relin_sched"], dict(B=20, nsteps=4, hold=2, traj_every=1), relin_data,
                  lambda api: api.call("f16_rollout_lqr_relin_sched", h_w=None, hold=2, **relin)))
    return c


CASES = _cases()
