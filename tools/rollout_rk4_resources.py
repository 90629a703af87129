"""Registers, scratch and LDS of the Runge-Kutta rollout kernels (f16_rollout_rk / _lqr_rk / _cost_rk) beside the Euler kernels they
are the twins of, as the compiler reports them: `hipcc -Rpass-analysis=kernel-resource-usage` over csrc/f16_dynamics.hip with the flags
of the default build (no GPU needed), once as the library is built and once with -DF16_RK4_512, which instantiates the 512-lane RK4
kernels that the launch rules leave out -- the evidence for leaving them out.  Writes profiles/rollout_rk4_resources.txt and fails
if a reachable RK4 instantiation has scratch or spills.

    python tools/rollout_rk4_resources.py
"""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from device_code import FIELDS, WIDTHS, remarks  # noqa: E402

VARIANT = {("false", "true", "false"): "open loop", ("true", "true", "false"): "LQR law", ("false", "true", "true"): "scored"}


def rows_of(found, reachable):
    """the scheduled rollout kernels of one compile: (kernel, <BLOCK, FI>, variant, stages, reachable, fields)"""
    rows = []
    for n, k in found.items():
        m = re.match(r"void f16::(k_rollout(?:_i|_exact)?)<(.*?)>\(", n)
        if not m:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        # k_rollout<BLOCK, FI, LQR, SCHED, COST, STAGES>, k_rollout_i<BLOCK, LQR, SCHED, COST, STAGES>, k_rollout_exact<LQR, SCHED, COST, STAGES>
        variant, stages = VARIANT.get(tuple(args[-4:-1])), int(args[-1])
        if variant:
            rows.append((m.group(1), ", ".join(args[:-4]), variant, stages, reachable, k))
    return rows


def main():
    rows = rows_of(remarks(REPO, "f16_dynamics.hip"), True)
    built = {r[:4] for r in rows}
    rows += [r[:4] + (False, r[5]) for r in rows_of(remarks(REPO, "f16_dynamics.hip", ["-DF16_RK4_512"]), True) if r[:4] not in built]
    rows.sort(key=lambda r: (r[0], [int(v) for v in r[1].split(",") if v.strip()], r[2], r[3]))
    out = os.path.join(REPO, "profiles", "rollout_rk4_resources.txt")
    bad = []
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, flags of the default build: the scheduled rollout kernels with the\n"
                "# Euler step (stages 1) and with the Runge-Kutta step (stages 4).  k_rollout<BLOCK, FI>: FI 0 = lofi, -1 = run-time flag;\n"
                "# k_rollout_i<BLOCK>: integer table image; k_rollout_exact: F16_FLAG_ONE_LANE (the step is an out-of-line function, whose\n"
                "# registers the caller's numbers include).  built = no: instantiated with -DF16_RK4_512 for this table alone -- the\n"
                "# launch rules never reach it, because it has scratch.  A workgroup of 512 lanes has 256 registers per lane, one of at\n"
                "# most 256 lanes has 512 (VGPR + AGPR).  static LDS limit of a workgroup: 163840 B\n")
        f.write(f"{'kernel':<16}{'<..>':<10}{'variant':<11}{'stages':>7}{'built':>6}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'scratch B/lane':>15}{'waves/SIMD':>11}"
                f"{'SGPR spill':>11}{'VGPR spill':>11}{'LDS B':>8}\n")
        for kern, targs, variant, stages, reachable, k in rows:
            f.write(f"{kern:<16}{targs:<10}{variant:<11}{stages:>7}{'yes' if reachable else 'no':>6}"
                    + "".join(f"{k.get(fl, 0):>{w}}" for fl, w in zip(FIELDS, WIDTHS)) + "\n")
            assert k.get("LDS Size [bytes/block]", 0) <= 163840, (kern, targs, variant)
            # k_rollout_exact calls its step: the compiler reserves a stack for the call (the step's own frame), which is no spill
            if stages == 4 and reachable and kern != "k_rollout_exact" and (k.get("ScratchSize [bytes/lane]", 0) or k.get("VGPRs Spill", 0)):
                bad.append((kern, targs, variant))
    print(open(out).read())
    assert not bad, f"reachable RK4 instantiations with scratch: {bad}"


if __name__ == "__main__":
    main()
