"""Registers, scratch and LDS of the soft-row instantiations of the one-wavefront MPC solver (f16_mpc_plan_soft_rows: k_mpc_wave_soft,
k_rollout_mpc_soft<RELIN>, and the out-of-line pieces run_iterations / terminate_test<ANYEQ, SOFT>) beside their hard twins, as the
compiler reports them: `hipcc -Rpass-analysis=kernel-resource-usage` over csrc/f16_mpc_wave.hip with the flags of the default build (no
GPU needed).  The hard twins are compiled a second time from the sources of the parent revision (git archive) and the figures compared:
the feature must not have changed them.  Writes profiles/mpc_soft_resources.txt; fails if a hard figure differs from the parent's or a
soft twin has another LDS size or occupancy than its hard twin, or scratch accesses inside the loops of run_iterations.

    python tools/mpc_soft_resources.py [--parent-rev HEAD~1]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from device_code import compiled, demangled, parent_tree, parse_remarks  # noqa: E402

COLUMNS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")
HEAD = ("SGPR", "VGPR", "AGPR", "scratch B/lane", "LDS B", "waves/SIMD", "SGPR spill", "VGPR spill")


def remarks(root):
    """{demangled name: {field: value}} of one compile of csrc/f16_mpc_wave.hip under `root` (kernels and out-of-line device functions)"""
    err, asm = compiled(root, "f16_mpc_wave.hip")
    funcs = parse_remarks(err)
    # the out-of-line device functions have no remark: their figures stand behind their code in the listing ("; Function info:")
    # -- and there is no spill count for them, so the scratch accesses inside their loops are counted instead (the hot loop: Depth >= 2)
    for m in re.finditer(r"\.Lfunc_end\d+:\n\t\.size\t(\S+), [^\n]*\n(?:[^\n]*\n){1,16}?; Function info:\n(.*?); MemoryBound", asm, flags=re.S):
        if "run_iterations" not in m.group(1) and "terminate_test" not in m.group(1):
            continue
        info = dict(re.findall(r"; (\w+): (\d+)", m.group(2)))
        body = asm[asm.index("\n" + m.group(1) + ":"):m.start()]
        hot, inloop = 0, False
        for ln in body.split("\n"):
            if ln.startswith(".LBB"):
                d = re.search(r"Depth=(\d+)", ln)
                inloop = bool(d) and int(d.group(1)) >= 2
            elif inloop and "scratch_" in ln:
                hot += 1
        funcs.append({"mangled": m.group(1), "TotalSGPRs": int(info["TotalNumSgprs"]), "VGPRs": int(info["NumVgprs"]), "AGPRs": int(info["NumAgprs"]),
                      "ScratchSize [bytes/lane]": int(info["ScratchSize"]), "hot": hot})
    return demangled(funcs)


def twin_key(name):
    """(family, template arguments without SOFT, soft) of a function this table lists, or None"""
    m = re.match(r"(?:void |int )?f16::wave::(k_mpc_wave|k_rollout_mpc)(_soft)?(?:<(\w+)>)?\(", name)
    if m:
        return m.group(1), m.group(3) or "", bool(m.group(2))
    m = re.match(r"(?:void |int )?f16::wave::(run_iterations|terminate_test)<(\w+)(?:, (\w+))?>\(", name)
    if m:      # <ANYEQ> (the parent) = <ANYEQ, false>
        return m.group(1), m.group(2), m.group(3) == "true"
    return None


def table(found):
    return {twin_key(n): k for n, k in found.items() if twin_key(n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-rev", default="HEAD~1", help="the revision whose hard kernels the figures are compared with")
    a = ap.parse_args()
    here = table(remarks(REPO))
    with tempfile.TemporaryDirectory() as tmp:
        parent = table(remarks(parent_tree(a.parent_rev, tmp)))
    rev = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", a.parent_rev], capture_output=True, text=True, check=True).stdout.strip()
    out = os.path.join(REPO, "profiles", "mpc_soft_resources.txt")
    bad = []
    fmt = lambda k: "".join(f"{k.get(fl, 0):>{w}}" for fl, w in zip(COLUMNS, (6, 6, 6, 15, 8, 11, 11, 11)))
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, flags of the default build, csrc/f16_mpc_wave.hip: every soft-row\n"
                "# instantiation (f16_mpc_plan_soft_rows) beside its hard twin, and the hard twin as the parent revision compiles it.  A kernel's\n"
                "# figures include those of the out-of-line functions it calls (factorise, run_iterations, terminate_test, ...); the two\n"
                "# functions that differ between hard and soft are listed on their own (<ANYEQ>: some row carries the 1e3 rho of an equality;\n"
                "# the compiler reports no LDS size, occupancy or spill count for a function that is no kernel: 0 there).\n"
                f"# parent = {rev}\n")
        f.write(f"{'function':<18}{'<..>':<7}{'rows':<8}" + "".join(f"{h:>{w}}" for h, w in zip(HEAD, (6, 6, 6, 15, 8, 11, 11, 11))) + "\n")
        for fam, targs in sorted({k[:2] for k in here}):
            hard, soft, par = here.get((fam, targs, False)), here.get((fam, targs, True)), parent.get((fam, targs, False))
            assert hard and soft and par, (fam, targs)
            note = lambda k: f"   scratch accesses inside its loops: {k['hot']}" if "hot" in k else ""
            f.write(f"{fam:<18}{targs:<7}{'hard':<8}{fmt(hard)}{note(hard)}\n{'':<18}{'':<7}{'parent':<8}{fmt(par)}{note(par)}\n"
                    f"{'':<18}{'':<7}{'soft':<8}{fmt(soft)}{note(soft)}\n")
            if soft.get("hot", 0):
                bad.append((fam, targs, "soft twin: scratch accesses inside a loop"))
            if any(hard.get(fl, 0) != par.get(fl, 0) for fl in COLUMNS):
                bad.append((fam, targs, "hard differs from the parent"))
            if fam.startswith("k_") and any(soft.get(fl, 0) != hard.get(fl, 0) for fl in ("LDS Size [bytes/block]", "Occupancy [waves/SIMD]")):
                bad.append((fam, targs, "soft twin: LDS size or occupancy"))
    print(open(out).read())
    assert not bad, bad


if __name__ == "__main__":
    main()
