"""Registers, scratch and LDS of every scheduled-gain rollout kernel (k_rollout_gs / k_rollout_i_gs / k_rollout_exact_gs,
f16_rollout_lqr_gs) beside the frozen-gain kernel it is the twin of (<LQR, SCHED>): `hipcc -Rpass-analysis=kernel-resource-usage`
over csrc/f16_dynamics.hip with the flags of the default build (no GPU needed).  In the same run the device assembly (`hipcc -S`) of
f16_dynamics.hip is compared with the parent commit's, function by function: every device function the parent has must be there
unchanged, instruction for instruction (labels renumbered, comments and directives dropped).  Writes
profiles/rollout_gs_resources.txt and fails if a new instantiation has scratch where its twin has none, more static LDS than a
workgroup can have, or if an existing function changed.

    python tools/rollout_gs_resources.py [--parent REV]      (REV defaults to HEAD while csrc/ or include/ differ from it, else HEAD~1)
"""
import argparse
import hashlib
import os
import re
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from device_code import FIELDS, WIDTHS, assembly, default_parent, parent_tree, remarks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    rev = default_parent(ap.parse_args().parent)
    found = remarks(REPO, "f16_dynamics.hip")
    new, twins = [], {}
    for n, k in found.items():
        m = re.match(r"void f16::k_rollout_gs<(-?\d+), (-?\d+), (\d+)>\(", n)
        if m:
            new.append(("k_rollout_gs", tuple(int(v) for v in m.groups()), k))
        m = re.match(r"void f16::k_rollout_i_gs<(\d+), (\d+)>\(", n)
        if m:
            new.append(("k_rollout_i_gs", tuple(int(v) for v in m.groups()), k))
        m = re.match(r"void f16::k_rollout_exact_gs<(\d+)>\(", n)
        if m:
            new.append(("k_rollout_exact_gs", (int(m.group(1)),), k))
        m = re.match(r"void f16::k_rollout<(-?\d+), (-?\d+), true, true, false, (\d+)>\(", n)
        if m:
            twins[("k_rollout_gs",) + tuple(int(v) for v in m.groups())] = ("k_rollout", k)
        m = re.match(r"void f16::k_rollout_i<(\d+), true, true, false, (\d+)>\(", n)
        if m:
            twins[("k_rollout_i_gs",) + tuple(int(v) for v in m.groups())] = ("k_rollout_i", k)
        m = re.match(r"void f16::k_rollout_exact<true, true, false, (\d+)>\(", n)
        if m:
            twins[("k_rollout_exact_gs", int(m.group(1)))] = ("k_rollout_exact", k)
    # 64 / 128 / 256 lanes x lofi / run-time fidelity x Euler / RK4, the 512-lane integer-image kernel (Euler), the flagged kernel x 2
    assert len(new) == 15, [f[:2] for f in new]
    new.sort(key=lambda f: (f[0], f[1]))
    with tempfile.TemporaryDirectory() as tmp:
        before = assembly(parent_tree(rev, tmp))
    after = assembly(REPO)
    changed = [f for f in before if before[f] != after.get(f)]
    digest = hashlib.sha256("\n".join(f + "\n" + "\n".join(before[f]) for f in sorted(before)).encode()).hexdigest()
    out = os.path.join(REPO, "profiles", "rollout_gs_resources.txt")
    bad = []
    row = lambda name, targs, k: f"{name:<22}{targs:<14}" + "".join(f"{k.get(fl, 0):>{w}}" for fl, w in zip(FIELDS, WIDTHS)) + "\n"
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, flags of the default build: every scheduled-gain rollout kernel and, under\n"
                "# it, its twin -- the frozen-gain kernel <LQR, SCHED> whose lane body it runs with the gain update added.\n"
                "# k_rollout_gs<BLOCK, FI, STAGES>: FI 0 = lofi, -1 = run-time flag; STAGES 1 = Euler, 4 = Runge-Kutta; twin\n"
                "# k_rollout<BLOCK, FI, true, true, false, STAGES>.  k_rollout_i_gs<BLOCK, STAGES>: integer table image, twin k_rollout_i<BLOCK, true,\n"
                "# true, false, STAGES>.  k_rollout_exact_gs<STAGES>: F16_FLAG_ONE_LANE, twin k_rollout_exact<true, true, false, STAGES>; both call\n"
                "# out-of-line steps, for whose frames the compiler reserves a stack (no spill).  static LDS limit of a workgroup: 163840 B\n")
        f.write(f"{'kernel':<22}{'<..>':<14}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'scratch B/lane':>15}{'waves/SIMD':>11}{'SGPR spill':>11}{'VGPR spill':>11}{'LDS B':>8}\n")
        for name, targs, k in new:
            tname, tk = twins[(name,) + targs]
            f.write(row(name, ", ".join(str(v) for v in targs), k))
            f.write(row("  " + tname, "(twin)", tk))
            assert k.get("LDS Size [bytes/block]", 0) <= 163840, (name, targs)
            if k.get("ScratchSize [bytes/lane]", 0) and not tk.get("ScratchSize [bytes/lane]", 0):
                bad.append((name, targs))
        f.write(f"\n# device assembly of csrc/f16_dynamics.hip against the parent commit, function by function (labels renumbered, comments and\n"
                f"# directives dropped): {len(before)} functions in the parent, {len(after)} now, {len(after) - len(before)} new;\n"
                f"# existing functions whose instructions changed: {len(changed)}" + ("" if not changed else " " + " ".join(sorted(changed))) + "\n"
                f"# sha256 of the parent's {len(before)} instruction streams: {digest}\n")
    print(open(out).read())
    assert not bad, f"scheduled-gain instantiations with scratch where the twin has none: {bad}"
    assert not changed, f"existing device functions changed: {changed}"


if __name__ == "__main__":
    main()
