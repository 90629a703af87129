"""The leading-dimension contract of include/f16_hip.h on the device: every case of tests/layout_cases.py goes through the C entry
points directly, once tight (ld = B, arrays allocated exactly) and once padded (odd ld >= B + 3, every array a view one element past
a 16-byte boundary inside a larger allocation, sentinels in guards, outputs and padding, FOREIGN in the status words of sticky
entries), from the same host inputs on the same stream; the padded call must equal the tight one bit for bit in the columns < B and
leave everything else as it was.  A third call with every optional output NULL must give the required outputs of the padded call.
Dispatch depends on B, not on ld, so both calls run the same kernel with the same work split: equality is the contract.  Nothing here
asserts accuracy -- the tight call's numbers are pinned by the rest of the suite.  States are tiled from 64 config-2 / config-4
states (fixed seeds); models and gains come from the existing calls, once per batch size."""
import contextlib
import ctypes

import numpy as np
import pytest

import layout_cases as lc

pytestmark = pytest.mark.gpu
EHIP = -2                              # F16_EHIP
BASE = 64                              # host states drawn once; larger batches tile them (altitude shifted per tile)


class Source:
    """states, models and gains of the cases: inputs here, not the thing under test"""
    mpc_x_idx = [3, 4, 7, 8, 9, 10, 11, 17, 16]

    def __init__(self):
        from f16_mpc_oop_py_amd import parameters
        from f16_mpc_oop_py_amd.workload import config2_states, config4_states
        assert list(parameters.mpc_x_idx) == self.mpc_x_idx
        self.x2, self.u2 = config2_states(BASE, seed=20261021)
        self.x4, self.u4 = config4_states(BASE, seed=2)          # (the smoke run's batch: feasible at these demands' scale)
        self._gain, self._model = None, {}

    @staticmethod
    def tile(a, B, shift_row=None):
        """[BASE, k] -> [k, B] state-major"""
        out = np.ascontiguousarray(a[np.arange(B) % len(a)].T)
        if shift_row is not None:
            out[shift_row] += 0.25 * (np.arange(B) // len(a))
        return out

    def states(self, B):
        return self.tile(self.x2, B, 2), self.tile(self.u2, B)

    def gain(self, B):
        """K [27, B] of the 64 base states (f16_lqr_batch through F16Batch), demands [3, B] that differ from column to column"""
        if self._gain is None:
            from f16_mpc_oop_py_amd import F16Batch
            self._gain = F16Batch(self.x2, self.u2, device="cuda:0")._calc_LQR_gain().reshape(BASE, 27).cpu().numpy()
        dem = np.array([[0.05], [-0.02], [0.01]]) * (1.0 + 0.1 * (np.arange(B) % 7))[None]
        return self.tile(self._gain, B), dem

    def model(self, B, kind):
        """"chain": config-2 states at xcg 0.25 with every stage of the control chain; "mpc" / "mpc3": config-4 states at xcg 0.35 with
        the reduced model discretised at 1 ms / 3 ms"""
        if (B, kind) not in self._model:
            import torch
            from f16_mpc_oop_py_amd import F16Batch
            host = lambda t: np.ascontiguousarray(t.cpu().numpy())
            if kind == "chain":
                x, u = self.x2[:B] if B <= BASE else self.x2[np.arange(B) % BASE], self.u2[:B] if B <= BASE else self.u2[np.arange(B) % BASE]
                env = F16Batch(x, u, xcg=0.25, device="cuda:0")
                K = env._calc_LQR_gain()
                Ad, Bd, Cd = env.ssr
                full = env.linearise_full(discretise=False)
                m = dict(Ac=host(env._lin[0]), Bc=host(env._lin[1]), K=host(K.reshape(B, 27).t()), Ac18=host(full["Ac"].reshape(B, 324).t()),
                         Bc18=host(full["Bc"].reshape(B, 72).t()))
            else:
                x, u = self.x4[:B], self.u4[:B]
                env = F16Batch(x, u, xcg=0.35, dt=0.003 if kind == "mpc3" else 0.001, device="cuda:0")
                Ad, Bd, Cd = env.build_ssr()
                m = {}
            torch.cuda.synchronize()
            m.update(x=np.ascontiguousarray(x.T), u=np.ascontiguousarray(u.T), Ad=host(Ad), Bd=host(Bd), Cd=host(Cd))
            self._model[(B, kind)] = m
        return self._model[(B, kind)]


class Api:
    """One call sequence of a case on one layout: the arrays on the device, every argument of a call taken by its header name"""

    def __init__(self, dev, case, bufs, B, ld, B0, ld0):
        self.dev, self.case, self.bufs, self.sizes = dev, case, bufs, dict(B=B, ld=ld, B0=B0, ld0=ld0)
        self.keep, self.hosts, self.tensors = [], {}, {}
        t = dev.torch
        for name, b in bufs.items():
            if b.null:
                continue
            d = t.from_numpy(b.full).to("cuda:0")
            assert d.data_ptr() % 16 == 0
            self.tensors[name] = d

    def ptr(self, name):
        b = self.bufs[name]
        if b.null:
            return None
        p = self.tensors[name].data_ptr() + b.off * b.itemsize
        assert not b.padded or p % 16 == b.itemsize           # one element past a 16-byte boundary
        return ctypes.c_void_p(p)

    def call(self, symbol, **given):
        from f16_mpc_oop_py_amd import cabi
        L, args = self.dev.L, []
        listed = {a.name for a in lc.ROWS[symbol].args}
        for _, p in cabi.functions()[symbol][1]:
            if p in given:
                args.append(given[p])
            elif p == "ctx":
                args.append(self.dev.ctx.handle)
            elif p == "stream":
                args.append(None)
            elif p in listed:
                args.append(self.ptr(p))
            else:
                args.append(self.sizes[p])
        rc = getattr(L, symbol)(*args)
        if rc == EHIP:                                        # nothing more is launched on a device that has faulted
            pytest.exit(f"{symbol} ({self.case.id}): {L.f16_last_error()}", returncode=3)
        assert rc == 0, (symbol, self.case.id, L.f16_last_error())

    # ---- what the cases hand over besides arrays
    def settings(self, **over):
        s = self.dev.lib.QPSettings()
        self.dev.L.f16_qp_default_settings(ctypes.byref(s))
        for k, v in over.items():
            setattr(s, k, v)
        self.keep.append(s)
        return ctypes.byref(s)

    def weights(self):
        w = self.dev.lib.MPCWeights()
        self.dev.L.f16_mpc_default_weights(ctypes.byref(w))
        self.keep.append(w)
        return ctypes.byref(w)

    def cost_weights(self):
        w = self.dev.lib.make_cost_weights(q=np.linspace(0.5, 1.5, 9), qf=np.linspace(2.0, 1.0, 9), r=[0.1, 0.2, 0.3], penalty=10.0)
        self.keep.append(w)
        return ctypes.byref(w)

    def gain_grid(self, h0, dh, v0, dv, nh, nv):
        g = self.dev.lib.GainGrid(h0, dh, v0, dv, nh, nv)
        self.keep.append(g)
        return ctypes.byref(g)

    def host(self, name, count):
        self.hosts[name] = np.full(count, np.nan)
        return self.hosts[name].ctypes.data_as(ctypes.c_void_p)

    @contextlib.contextmanager
    def plan(self, create, hzn, dt):
        h, L = ctypes.c_void_p(), self.dev.L
        extra = dict(h_w=self.weights()) if create.endswith("_w") else {}
        self.call(create, plan=ctypes.byref(h), hzn=hzn, dt=dt, s=self.settings(), **extra)
        try:
            yield h
        finally:
            L.f16_mpc_plan_destroy(h)

    def warm_start(self, plan):
        assert self.dev.L.f16_mpc_plan_warm_start(plan, 1) == 0, self.dev.L.f16_last_error()

    def soft_rows(self, plan, w9):
        assert self.dev.L.f16_mpc_plan_soft_rows(plan, (ctypes.c_double * 9)(*w9)) == 0, self.dev.L.f16_last_error()

    def finish(self):
        try:
            self.dev.torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"{self.case.id}: {e}", returncode=3)
        for name, d in self.tensors.items():
            self.bufs[name].after = d.cpu().numpy()
        return self.bufs


class Dev:
    def __init__(self):
        import torch
        from f16_mpc_oop_py_amd import lib
        self.torch, self.lib, self.L = torch, lib, lib.load()
        self.ctx = lib.Context(0)
        self.src = Source()


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


def run(dev, case, data, padded, bare=False):
    n = case.n
    bufs, ld, ld0 = lc.layout(case.args(), n, n["B"], n["B0"], padded, data, case.status_rule(), bare)
    api = Api(dev, case, bufs, n["B"], ld, n["B0"], ld0)
    case.run(api)
    return api.finish(), api.hosts


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_the_padded_call_equals_the_tight_call(dev, case):
    data = case.data(dev.src, case.n)
    args, rule = case.args(), case.status_rule()
    tight, th = run(dev, case, data, False)
    padded, ph = run(dev, case, data, True)
    wrote = [a.name for a in args if a.role != "in" and not (a.name == "status" and rule == "sticky")
             and (tight[a.name].after != tight[a.name].before).any()]
    assert wrote or th, "the tight call wrote nothing"
    for k in wrote:                                           # (not a statement about accuracy: the call did its work and left numbers)
        b = tight[k]
        assert not b.f8 or np.isfinite(b.view(b.after).view(np.float64)[:, :b.B]).any(), f"{k}: nothing finite came back"
    bad = lc.compare(args, rule, tight, padded)
    for k in th:                                              # (the QP on the host: the same bits from either layout)
        assert not np.isnan(th[k]).all() and np.array_equal(th[k].view(np.int64), ph[k].view(np.int64)), k
    if any(a.optional and a.role != "in" for a in args):
        bare, _ = run(dev, case, data, True, bare=True)
        bad += lc.compare_required(args, padded, bare)
    assert not bad, (case.id, bad)
