"""oracle/lin_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

ctypes view of the batched linearisation entries of oracle/f16_oracle.c, for any of its three builds (oracle/Makefile):

  libf16_oracle.so      fp64, the restatement every fixture pins
  libf16_oracle_fma.so  fp64 with FMA contraction: the same rule under other rounding
  libf16_oracle_ld.so   `long double` (x87 extended precision): the reference of tests/linearise_cases.py

The matrices come back in the type the build computes in (numpy float64 or longdouble), never rounded on the way.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fp64": "libf16_oracle.so", "fma": "libf16_oracle_fma.so", "ld": "libf16_oracle_ld.so"}
TABLE_IMAGE_LEN = 5 * 20 + 13405 + 108 + 4 * 84 + 2 * 84 + 2 * 60 + 12


class LinOracle:
    def __init__(self, build="fp64", path=None):
        path = path or os.path.join(HERE, LIBS[build])
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path}: run `make -C oracle {os.path.basename(path)}`")
        L = self.lib = ctypes.CDLL(path)
        L.f16o_real_bytes.restype = ctypes.c_int
        nbytes = L.f16o_real_bytes()
        self.dtype = np.dtype(np.float64) if nbytes == 8 else np.dtype(np.longdouble)
        if self.dtype.itemsize != nbytes:
            raise RuntimeError(f"{path} computes in a {nbytes}-byte type numpy has no name for on this machine")
        vp, d, i, l = ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_long
        for f in (L.f16o_linearise_na_batch, L.f16o_linearise_full_batch):
            f.argtypes = [vp, vp, l, d, vp, vp, vp, vp, i, d]
            f.restype = None
        L.f16o_table_image.argtypes = [vp, l]
        L.f16o_table_image.restype = l
        L.f16o_set_fix_clr.argtypes = [i]
        L.f16o_last_status.restype = i
        dp = ctypes.POINTER(d)
        L.f16o_calc_xdot.argtypes = [dp, dp, dp, i, d]
        L.f16o_calc_xdot_na.argtypes = [dp, dp, dp, dp, i, d]
        L.f16o_init.restype = None
        L.f16o_init()

    def set_fix_clr(self, on):
        self.lib.f16o_set_fix_clr(int(on))

    def table_image(self):
        """breakpoints [5][20] | hifi tables | lofi tables, as this build holds them"""
        out = np.zeros(TABLE_IMAGE_LEN, self.dtype)
        n = self.lib.f16o_table_image(out.ctypes.data, len(out))
        assert n == len(out), n
        return out

    def _lin(self, fn, ns, ni, no, x, u, eps, fi_flag, xcg):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 18)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 4)
        B = len(x)
        assert len(u) == B
        A, Bm, C = np.zeros((B, ns, ns), self.dtype), np.zeros((B, ns, ni), self.dtype), np.zeros((B, no, ns), self.dtype)
        st = np.zeros(B, np.int32)
        fn(x.ctypes.data, u.ctypes.data, B, float(eps), A.ctypes.data, Bm.ctypes.data, C.ctypes.data, st.ctypes.data, int(fi_flag),
           float(xcg))
        return A, Bm, C, st

    def linearise_na_batch(self, x, u, eps=1e-5, fi_flag=1, xcg=0.25):
        """x [B,18], u [B,4] -> A [B,9,9], Bm [B,9,3], C [B,9,9], status [B] (the OR over all 13 evaluated points)"""
        return self._lin(self.lib.f16o_linearise_na_batch, 9, 3, 9, x, u, eps, fi_flag, xcg)

    def linearise_full_batch(self, x, u, eps=1e-5, fi_flag=1, xcg=0.25):
        """x [B,18], u [B,4] -> A [B,18,18], Bm [B,18,4], C [B,10,18], status [B] (the OR over all 23 evaluated points)"""
        return self._lin(self.lib.f16o_linearise_full_batch, 18, 4, 10, x, u, eps, fi_flag, xcg)

    def status_at(self, x, u, fi_flag, xcg, reduced):
        """grid-clamp bits of ONE plant evaluation at (x [18], u [4]): f16o_calc_xdot, or f16o_calc_xdot_na at x9 = x[mpc idx],
        u3 = u[1:4], then f16o_last_status"""
        dp = ctypes.POINTER(ctypes.c_double)
        x = np.ascontiguousarray(x, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.zeros(18)
        if reduced:
            x9, u3 = np.ascontiguousarray(x[[3, 4, 7, 8, 9, 10, 11, 17, 16]]), np.ascontiguousarray(u[1:4])
            self.lib.f16o_calc_xdot_na(x.ctypes.data_as(dp), x9.ctypes.data_as(dp), u3.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                       int(fi_flag), float(xcg))
        else:
            self.lib.f16o_calc_xdot(x.ctypes.data_as(dp), u.ctypes.data_as(dp), out.ctypes.data_as(dp), int(fi_flag), float(xcg))
        return self.lib.f16o_last_status()
