"""Registers, scratch and LDS of the scored rollout kernels (f16_rollout_cost) beside the scheduled kernels they are built from, as
the compiler reports them: one `hipcc -Rpass-analysis=kernel-resource-usage` pass over csrc/f16_dynamics.hip with the flags of the
default build (no GPU needed).  Writes profiles/rollout_cost_resources.txt.

    python tools/rollout_cost_resources.py
"""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from f16_mpc_oop_py_amd import lib  # noqa: E402

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def main():
    src = os.path.join(lib.CSRC, "f16_dynamics.hip")
    flags = [f for f in lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                                         "-o", os.path.join(tmp, "dyn.s"), src]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    kernels, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1)}
            kernels.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    names = subprocess.run(["c++filt"], input="\n".join(k["mangled"] for k in kernels), capture_output=True, text=True, check=True).stdout.split("\n")
    rows = []
    for k, n in zip(kernels, names):
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
            f.write(f"{kern:<16}{targs:<10}{variant:<11}" + "".join(f"{k.get(fl, 0):>{w}}" for fl, w in zip(FIELDS, (5, 5, 5, 15, 11, 11, 11, 8))) + "\n")
            assert k.get("LDS Size [bytes/block]", 0) <= 163840, (kern, targs, variant)
    print(open(out).read())


if __name__ == "__main__":
    main()
