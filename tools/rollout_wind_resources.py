"""Registers, scratch and LDS of the wind kernels (csrc/f16_wind.hip: k_rollout_wind, k_rollout_wind_exact, k_xdot_wind, k_gust_sample;
csrc/f16_wind_ens.hip: their ensemble twins k_rollout_wind_ens, k_rollout_wind_exact_ens and k_ens_from_traj, k_ens_finish) as
the compiler reports them (`hipcc -Rpass-analysis=kernel-resource-usage`, flags of the default build, no GPU needed), beside the
still-air kernel each rollout kernel is the twin of (k_rollout<BLOCK, -1, LQR, true, false, STAGES> / k_rollout_exact<LQR, true, false,
STAGES> of csrc/f16_dynamics.hip).  In the same run every rollout kernel of f16_dynamics.hip is held against the parent commit's
sources: the same SGPR / VGPR / AGPR / scratch / LDS figures, and the same device assembly function by function (labels renumbered,
comments and directives dropped) -- the wind kernels are a translation unit of their own, and what they share with the existing ones
moved into a header without touching an instruction.  Writes profiles/rollout_wind_resources.txt and fails if an existing kernel
changed, if a wind kernel has more static LDS than a workgroup can have, or if a reachable wind kernel (other than the flagged one,
which calls its step) has scratch memory.

    python tools/rollout_wind_resources.py [--parent REV]      (REV defaults to HEAD while csrc/ or include/ differ from it, else HEAD~1)
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
    with tempfile.TemporaryDirectory() as tmp:
        parent = parent_tree(rev, tmp)
        dyn_before, asm_before = remarks(parent, "f16_dynamics.hip"), assembly(parent)
    dyn, asm_after = remarks(REPO, "f16_dynamics.hip"), assembly(REPO)
    wind = remarks(REPO, "f16_wind.hip")
    rollouts = sorted(n for n in dyn_before if "k_rollout" in n)
    moved = [n for n in rollouts if dyn_before[n] != dyn.get(n)]
    asm_wind = assembly(REPO, "f16_wind.hip")
    ens, asm_ens = remarks(REPO, "f16_wind_ens.hip"), assembly(REPO, "f16_wind_ens.hip")
    for found, asm in ((wind, asm_wind), (dyn, asm_after), (ens, asm_ens)):          # instructions of each kernel's own body, as emitted
        for k in found.values():
            k["instr"] = len(asm.get(k["mangled"], ()))
    changed = [f for f in asm_before if asm_before[f] != asm_after.get(f)]
    digest = hashlib.sha256("\n".join(f + "\n" + "\n".join(asm_before[f]) for f in sorted(asm_before)).encode()).hexdigest()
    rows, bad = [], []
    for n, k in wind.items():
        m = re.match(r"void f16::k_rollout_wind<(\d+), (true|false), (\d+)>\(", n)
        if m:
            blk, lqr, stg = int(m.group(1)), m.group(2), int(m.group(3))
            rows.append(("k_rollout_wind", (blk, lqr == "true", stg), k, f"void f16::k_rollout<{blk}, -1, {lqr}, true, false, {stg}>("))
            continue
        m = re.match(r"void f16::k_rollout_wind_exact<(true|false), (\d+)>\(", n)
        if m:
            rows.append(("k_rollout_wind_exact", (0, m.group(1) == "true", int(m.group(2))), k,
                         f"void f16::k_rollout_exact<{m.group(1)}, true, false, {m.group(2)}>("))
            continue
        m = re.match(r"void f16::(k_xdot_wind|k_gust_sample)(?:<(\d+)>)?\(", n)
        if m:
            rows.append((m.group(1), (int(m.group(2) or 64), False, 0), k, f"void f16::k_xdot<{m.group(2)}, -1>(" if m.group(2) else None))
    rows.sort(key=lambda r: (r[0], r[1]))
    assert len([r for r in rows if r[0] == "k_rollout_wind"]) == 12 and len([r for r in rows if r[0] == "k_rollout_wind_exact"]) == 4, [r[:2] for r in rows]
    out = os.path.join(REPO, "profiles", "rollout_wind_resources.txt")
    line = lambda name, targs, k: f"{name:<24}{targs:<18}" + "".join(f"{k[fl]:>{w}}" for fl, w in zip(FIELDS, WIDTHS)) + f"{k['instr']:>8}\n"
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, flags of the default build: every kernel of csrc/f16_wind.hip and, under\n"
                "# it, the still-air kernel of csrc/f16_dynamics.hip it is the twin of.  k_rollout_wind<BLOCK, LQR, STAGES> (STAGES 1 = Euler,\n"
                "# 4 = Runge-Kutta; run-time fidelity), twin k_rollout<BLOCK, -1, LQR, true, false, STAGES>; k_rollout_wind_exact<LQR, STAGES>:\n"
                "# F16_FLAG_ONE_LANE, twin k_rollout_exact<LQR, true, false, STAGES> -- both call out-of-line steps, for whose frames the compiler\n"
                "# reserves a stack; the out-of-line Runge-Kutta wind step itself spills a few registers there (VGPR spill): the price of a step\n"
                "# that is one instruction sequence for every caller.  A workgroup of at most 256 lanes has 512 registers per lane (VGPR + AGPR).\n"
                "# scratch B/lane = 0: nothing of the kernel reaches memory but its loads and stores.  instr: instructions of the kernel body as\n"
                "# emitted (the flagged kernels: without the out-of-line step).  static LDS limit of a workgroup: 163840 B\n")
        f.write(f"{'kernel':<24}{'<..>':<18}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'scratch B/lane':>15}{'waves/SIMD':>11}{'SGPR spill':>11}{'VGPR spill':>11}{'LDS B':>8}{'instr':>8}\n")
        for name, targs, k, twin in rows:
            shown = ", ".join(str(v).lower() for v in (targs if name == "k_rollout_wind" else targs[1:] if name == "k_rollout_wind_exact" else targs[:1]))
            f.write(line(name, shown, k))
            if twin:
                tk = next(v for n, v in dyn.items() if n.startswith(twin))
                f.write(line("  " + twin.split("::")[1].split("<")[0], "(twin)", tk))
            assert k["LDS Size [bytes/block]"] <= 163840, (name, targs)
            if name != "k_rollout_wind_exact" and k["ScratchSize [bytes/lane]"]:
                bad.append((name, targs))
        # the ensemble twins (csrc/f16_wind_ens.hip), each under the kernel of csrc/f16_wind.hip it is the twin of: recorded, not judged
        erows = []
        for n, k in ens.items():
            m = re.match(r"void f16::k_rollout_wind_ens<(\d+), (true|false), (\d+)>\(", n)
            if m:
                erows.append(("k_rollout_wind_ens", (int(m.group(1)), m.group(2) == "true", int(m.group(3))), k,
                              f"void f16::k_rollout_wind<{m.group(1)}, {m.group(2)}, {m.group(3)}>("))
                continue
            m = re.match(r"void f16::k_rollout_wind_exact_ens<(true|false), (\d+)>\(", n)
            if m:
                erows.append(("k_rollout_wind_exact_ens", (m.group(1) == "true", int(m.group(2))), k,
                              f"void f16::k_rollout_wind_exact<{m.group(1)}, {m.group(2)}>("))
                continue
            m = re.match(r"f16::(k_ens_from_traj|k_ens_finish)\(", n)
            if m:
                erows.append((m.group(1), (), k, None))
        erows.sort(key=lambda r: (r[0], r[1]))
        assert len([r for r in erows if r[0] == "k_rollout_wind_ens"]) == 12 and len([r for r in erows if r[0] == "k_rollout_wind_exact_ens"]) == 4 \
            and len(erows) == 18, [r[:2] for r in erows]
        f.write("\n# the ensemble twins of csrc/f16_wind_ens.hip (the ENS lane loop: the wave's records of every sample formed in registers),\n"
                "# each above the kernel of csrc/f16_wind.hip it is the twin of (k_rollout_wind_exact_e. = k_rollout_wind_exact_ens); k_ens_from_traj\n"
                "# and k_ens_finish have none.  Recorded, not judged: k_rollout_wind_ens<*, false, 4> spills 4 vector registers (32 B / lane)\n")
        for name, targs, k, twin in erows:
            f.write(line({"k_rollout_wind_exact_ens": "k_rollout_wind_exact_e."}.get(name, name), ", ".join(str(v).lower() for v in targs), k))
            if twin:
                f.write(line("  " + twin.split("::")[1].split("<")[0], "(twin)", next(v for n, v in wind.items() if n.startswith(twin))))
            assert k["LDS Size [bytes/block]"] <= 163840, (name, targs)
        f.write(f"\n# the {len(rollouts)} rollout kernels of csrc/f16_dynamics.hip against the parent commit's sources: SGPR / VGPR / AGPR / scratch / spill /\n"
                f"# LDS figures that differ: {len(moved)}" + ("" if not moved else " " + " ".join(moved)) + "\n"
                f"# device assembly of csrc/f16_dynamics.hip against the parent commit, function by function (labels renumbered, comments and\n"
                f"# directives dropped): {len(asm_before)} functions in the parent, {len(asm_after)} now;\n"
                f"# existing functions whose instructions changed: {len(changed)}" + ("" if not changed else " " + " ".join(sorted(changed))) + "\n"
                f"# sha256 of the parent's {len(asm_before)} instruction streams: {digest}\n")
    print(open(out).read())
    assert not moved and not changed, f"existing kernels changed: {moved} {changed}"
    assert not bad, f"wind kernels with scratch or spills: {bad}"


if __name__ == "__main__":
    main()
