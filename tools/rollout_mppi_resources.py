"""Registers, scratch and LDS of every instantiation of the fused MPPI loop (k_rollout_mppi / k_rollout_mppi_exact, f16_rollout_mppi)
beside the scored rollout kernel whose lane body it runs -- its twin: `hipcc -Rpass-analysis=kernel-resource-usage` over
csrc/f16_dynamics.hip with the flags of the default build (no GPU needed).  Writes profiles/rollout_mppi_resources.txt and fails if a
fused instantiation has scratch where its twin has none, or more static LDS than a workgroup can have.

    python tools/rollout_mppi_resources.py
"""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from device_code import FIELDS, WIDTHS, remarks  # noqa: E402


def main():
    found = remarks(REPO, "f16_dynamics.hip")
    fused, twins = [], {}
    for n, k in found.items():
        m = re.match(r"void f16::k_rollout_mppi<(-?\d+), (-?\d+), (\d+)>\(", n)
        if m:
            fused.append(("k_rollout_mppi", tuple(int(v) for v in m.groups()), k))
        m = re.match(r"void f16::k_rollout_mppi_exact<(\d+)>\(", n)
        if m:
            fused.append(("k_rollout_mppi_exact", (int(m.group(1)),), k))
        m = re.match(r"void f16::k_rollout<(-?\d+), (-?\d+), false, true, true, (\d+)>\(", n)      # the scored kernels
        if m:
            twins[("k_rollout_mppi",) + tuple(int(v) for v in m.groups())] = ("k_rollout", k)
        m = re.match(r"void f16::k_rollout_exact<false, true, true, (\d+)>\(", n)
        if m:
            twins[("k_rollout_mppi_exact", int(m.group(1)))] = ("k_rollout_exact", k)
    assert len(fused) == 14, [f[:2] for f in fused]
    fused.sort(key=lambda f: (f[0], f[1]))
    out = os.path.join(REPO, "profiles", "rollout_mppi_resources.txt")
    bad = []
    row = lambda name, targs, k: f"{name:<22}{targs:<14}" + "".join(f"{k.get(fl, 0):>{w}}" for fl, w in zip(FIELDS, WIDTHS)) + "\n"
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, flags of the default build: every instantiation of the fused MPPI loop\n"
                "# and, under it, its twin -- the scored rollout kernel whose lane body it runs.  k_rollout_mppi<BLOCK, FI, STAGES>: FI 0 = lofi,\n"
                "# -1 = run-time flag; STAGES 1 = Euler, 4 = Runge-Kutta; twin k_rollout<BLOCK, FI, false, true, true, STAGES>.\n"
                "# k_rollout_mppi_exact<STAGES>: F16_FLAG_ONE_LANE, twin k_rollout_exact<false, true, true, STAGES>; both call out-of-line steps,\n"
                "# for whose frames the compiler reserves a stack (no spill).  static LDS limit of a workgroup: 163840 B\n")
        f.write(f"{'kernel':<22}{'<..>':<14}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'scratch B/lane':>15}{'waves/SIMD':>11}{'SGPR spill':>11}{'VGPR spill':>11}{'LDS B':>8}\n")
        for name, targs, k in fused:
            tname, tk = twins[(name,) + targs]
            f.write(row(name, ", ".join(str(v) for v in targs), k))
            f.write(row("  " + tname, "(twin)", tk))
            assert k.get("LDS Size [bytes/block]", 0) <= 163840, (name, targs)
            if k.get("ScratchSize [bytes/lane]", 0) and not tk.get("ScratchSize [bytes/lane]", 0):
                bad.append((name, targs))
    print(open(out).read())
    assert not bad, f"fused instantiations with scratch where the twin has none: {bad}"


if __name__ == "__main__":
    main()
