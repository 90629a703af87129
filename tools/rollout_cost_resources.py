"""Registers, scratch and LDS of the scored rollout kernels (f16_rollout_cost) beside the scheduled kernels they are built from, as
the compiler reports them: one `hipcc -Rpass-analysis=kernel-resource-usage` pass over csrc/f16_dynamics.hip with the flags of the
default build (no GPU needed).  Writes profiles/rollout_cost_resources.txt.

    python tools/rollout_cost_resources.py
"""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from device_code import FIELDS, WIDTHS, remarks  # noqa: E402


def main():
    rows = []
    for n, k in remarks(REPO, "f16_dynamics.hip").items():
        m = re.match(r"void f16::(k_rollout(?:_i|_exact)?)<(.*?)>\(", n)
        if not m:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        # k_rollout<BLOCK, FI, LQR, SCHED, COST, STAGES>, k_rollout_i<BLOCK, LQR, SCHED, COST, STAGES>, k_rollout_exact<LQR, SCHED, COST, STAGES>
        # (STAGES 1: the Euler step; the Runge-Kutta twins have a table of their own, tools/rollout_rk4_resources.py)
        lqr, sched, cost, stages = args[-4:]
        if lqr == "false" and sched == "true" and stages == "1":
            rows.append((m.group(1), ", ".join(args[:-4]), "scored" if cost == "true" else "scheduled", k))
    rows.sort(key=lambda r: (r[0], [int(v) for v in r[1].split(",") if v.strip()], r[2]))
    out = os.path.join(REPO, "profiles", "rollout_cost_resources.txt")
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, flags of the default build; the open-loop scheduled kernels\n"
                "# (f16_rollout_sched) and their scored twins (f16_rollout_cost).  k_rollout<BLOCK, FI>: FI 0 = lofi, -1 = run-time flag.\n"
                "# static LDS limit of a workgroup: 163840 B\n")
        f.write(f"{'kernel':<16}{'<..>':<10}{'variant':<11}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'scratch B/lane':>15}{'waves/SIMD':>11}"
                f"{'SGPR spill':>11}{'VGPR spill':>11}{'LDS B':>8}\n")
        for kern, targs, variant, k in rows:
            f.write(f"{kern:<16}{targs:<10}{variant:<11}" + "".join(f"{k.get(fl, 0):>{w}}" for fl, w in zip(FIELDS, WIDTHS)) + "\n")
            assert k.get("LDS Size [bytes/block]", 0) <= 163840, (kern, targs, variant)
    print(open(out).read())


if __name__ == "__main__":
    main()
