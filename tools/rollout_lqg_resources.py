"""Registers, scratch and LDS of the output-feedback kernels (csrc/f16_observer.hip: k_rollout_lqg_wind, k_rollout_lqg_wind_exact,
k_observer_step, k_kalman) as the compiler reports them (`hipcc -Rpass-analysis=kernel-resource-usage`, flags of the default build,
no GPU needed), each rollout twin above the kernel of csrc/f16_wind.hip / csrc/f16_wind_ens.hip it extends.  In the same run every
function of csrc/f16_wind.hip, csrc/f16_wind_ens.hip and csrc/f16_control.hip is held against the parent commit's sources: the same
resource figures and the same device assembly function by function (labels renumbered, comments and directives dropped) -- the OBS
template parameter of the lane loop (csrc/f16_wind_lanes.hpp) and the second doubling function leave the existing instantiations
what they were.  Writes profiles/rollout_lqg_resources.txt and fails if an existing function changed, if a twin has more static LDS
than a workgroup can have, or if a default twin (other than the flagged ones, which call their step) has scratch memory.

    python tools/rollout_lqg_resources.py [--parent REV]      (REV defaults to HEAD while csrc/ or include/ differ from it, else HEAD~1)
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

EXISTING = ("f16_wind.hip", "f16_wind_ens.hip", "f16_control.hip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    rev = default_parent(ap.parse_args().parent)
    before, after, asm_before, asm_after = {}, {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        parent = parent_tree(rev, tmp)
        for name in EXISTING:
            before[name], asm_before[name] = remarks(parent, name), assembly(parent, name)
    for name in EXISTING:
        after[name], asm_after[name] = remarks(REPO, name), assembly(REPO, name)
    obs, asm_obs = remarks(REPO, "f16_observer.hip"), assembly(REPO, "f16_observer.hip")
    for k in obs.values():
        k["instr"] = len(asm_obs.get(k["mangled"], ()))
    for name in EXISTING:
        for k in after[name].values():
            k["instr"] = len(asm_after[name].get(k["mangled"], ()))
    figures = lambda k: {f: k[f] for f in FIELDS}
    moved = [f"{name}: {n}" for name in EXISTING for n, k in before[name].items() if n not in after[name] or figures(k) != figures(after[name][n])]
    changed = [f"{name}: {f}" for name in EXISTING for f in asm_before[name] if asm_before[name][f] != asm_after[name].get(f)]
    rows, bad = [], []
    for n, k in obs.items():
        m = re.match(r"void f16::k_rollout_lqg_wind<(\d+), (\d+), (true|false)>\(", n)
        if m:
            blk, stg, ens = int(m.group(1)), int(m.group(2)), m.group(3) == "true"
            twin = (f"void f16::k_rollout_wind_ens<{blk}, true, {stg}>(", "f16_wind_ens.hip") if ens else (f"void f16::k_rollout_wind<{blk}, true, {stg}>(", "f16_wind.hip")
            rows.append(("k_rollout_lqg_wind", (ens, blk, stg), k, twin))
            continue
        m = re.match(r"void f16::k_rollout_lqg_wind_exact<(\d+), (true|false)>\(", n)
        if m:
            stg, ens = int(m.group(1)), m.group(2) == "true"
            twin = (f"void f16::k_rollout_wind_exact_ens<true, {stg}>(", "f16_wind_ens.hip") if ens else (f"void f16::k_rollout_wind_exact<true, {stg}>(", "f16_wind.hip")
            rows.append(("k_rollout_lqg_wind_exact", (ens, stg), k, twin))
            continue
        m = re.match(r"f16::(k_observer_step|k_kalman)\(", n)
        if m:
            rows.append((m.group(1), (), k, (("f16::k_lqr(", "f16_control.hip") if m.group(1) == "k_kalman" else None)))
    rows.sort(key=lambda r: (r[0], r[1]))
    assert len([r for r in rows if r[0] == "k_rollout_lqg_wind"]) == 12 and len([r for r in rows if r[0] == "k_rollout_lqg_wind_exact"]) == 4 \
        and len(rows) == 18, [r[:2] for r in rows]
    digest = hashlib.sha256("\n".join(name + "\n" + f + "\n" + "\n".join(asm_before[name][f]) for name in EXISTING for f in sorted(asm_before[name])).encode()).hexdigest()
    out = os.path.join(REPO, "profiles", "rollout_lqg_resources.txt")
    line = lambda name, targs, k: f"{name:<26}{targs:<18}" + "".join(f"{k[fl]:>{w}}" for fl, w in zip(FIELDS, WIDTHS)) + f"{k['instr']:>8}\n"
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, flags of the default build: every kernel of csrc/f16_observer.hip and, under\n"
                "# it, the kernel it extends.  k_rollout_lqg_wind<BLOCK, STAGES, ENS> (STAGES 1 = Euler, 4 = Runge-Kutta), shown as ens, BLOCK, STAGES:\n"
                "# twin k_rollout_wind<BLOCK, true, STAGES> or k_rollout_wind_ens<...>; k_rollout_lqg_wind_exact<STAGES, ENS> (F16_FLAG_ONE_LANE), shown\n"
                "# as ens, STAGES: twin k_rollout_wind_exact<true, STAGES> or its _ens -- these call the out-of-line step and the out-of-line\n"
                "# observer_update, for whose frames the compiler reserves a stack; so does k_observer_step (8 B / lane: one saved register of\n"
                "# observer_update).  The default twins inline both: scratch B/lane = 0, nothing of them reaches memory but their loads and\n"
                "# stores -- the prediction lives in the xhat array between steps.  A workgroup of at most 256 lanes has 512 registers per\n"
                "# lane (VGPR + AGPR).  instr: instructions of the kernel body as emitted.  static LDS limit of a workgroup: 163840 B\n")
        f.write(f"{'kernel':<26}{'<..>':<18}{'VGPR':>5}{'AGPR':>5}{'SGPR':>5}{'scratch B/lane':>15}{'waves/SIMD':>11}{'SGPR spill':>11}{'VGPR spill':>11}{'LDS B':>8}{'instr':>8}\n")
        for name, targs, k, twin in rows:
            f.write(line(name, ", ".join(str(v).lower() for v in targs), k))
            if twin:
                f.write(line("  " + twin[0].split("::")[1].split("<")[0].split("(")[0], "(twin)", next(v for n, v in after[twin[1]].items() if n.startswith(twin[0]))))
            assert k["LDS Size [bytes/block]"] <= 163840, (name, targs)
            if name == "k_rollout_lqg_wind" and k["ScratchSize [bytes/lane]"]:
                bad.append((name, targs))
        nb = sum(len(v) for v in asm_before.values())
        f.write(f"\n# csrc/{', csrc/'.join(EXISTING)} against the parent commit's sources:\n"
                f"# kernels whose SGPR / VGPR / AGPR / scratch / spill / LDS figures differ: {len(moved)}" + ("" if not moved else " " + "; ".join(moved)) + "\n"
                f"# device assembly function by function (labels renumbered, comments and directives dropped): {nb} functions in the parent,\n"
                f"# {sum(len(v) for v in asm_after.values())} now; existing functions whose instructions changed: {len(changed)}" + ("" if not changed else " " + "; ".join(sorted(changed))) + "\n"
                f"# sha256 of the parent's {nb} instruction streams: {digest}\n")
    print(open(out).read())
    assert not moved and not changed, f"existing kernels changed: {moved} {changed}"
    assert not bad, f"default twins with scratch memory: {bad}"


if __name__ == "__main__":
    main()
