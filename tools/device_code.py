"""The device code of csrc files as the compiler emits it (no GPU needed): what the *_resources.py report tools share, and the check
"the same device code as the parent commit" as a command line.  One device-only compile of a file (`hipcc -S
-Rpass-analysis=kernel-resource-usage`, flags of the default build) gives the resource figures of its kernels (remarks) and the
instruction stream of every device function (assembly: labels renumbered, comments and directives dropped).

    python tools/device_code.py f16_dynamics.hip f16_wind.hip ... [--parent REV] [--allow-new]

names every device function of these files that is missing, new (an error unless --allow-new), or differs from REV's in instructions
or resource figures -- with the figures of each such function before -> after -- and exits non-zero if there is one.  REV defaults to HEAD while csrc/ or include/ differ from it, else HEAD~1."""
import argparse
import functools
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from f16_mpc_oop_py_amd import lib  # noqa: E402

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
WIDTHS = (5, 5, 5, 15, 11, 11, 11, 8)
CSRC = os.path.join("f16_mpc_oop_py_amd", "csrc")


@functools.lru_cache(maxsize=None)
def compiled(root, name, extra=()):
    """(the compiler's remarks, the assembly listing) of csrc/<name> under the tree `root`, compiled once per process"""
    flags = [f for f in lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + list(extra)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                                         "-o", out, os.path.join(root, CSRC, name)]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        return err, open(out).read()


def parse_remarks(err):
    """[{"mangled": symbol, field: value}] of the kernels in the compiler's remarks, in their order"""
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
    return kernels


def demangled(funcs):
    """{demangled name: entry} of entries with a "mangled" symbol"""
    names = subprocess.run(["c++filt"], input="\n".join(k["mangled"] for k in funcs), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, funcs))


def remarks(root, name, extra=()):
    """{demangled kernel name: {field: value, "mangled": symbol}} of csrc/<name> under `root`; a figure the compiler leaves out is 0"""
    return demangled([dict({f: k.get(f, 0) for f in FIELDS}, mangled=k["mangled"]) for k in parse_remarks(compiled(root, name, tuple(extra))[0])])


def assembly(root, name="f16_dynamics.hip"):
    """{function symbol: [instruction lines]} of csrc/<name> under `root`"""
    text = compiled(root, name)[1]
    symbols = set(re.findall(r"^\s*\.type\s+([\w.$]+),@function", text, re.M))
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"([A-Za-z_][\w.$]*):", line)
        if m and m.group(1) in symbols:
            cur = m.group(1)
            funcs[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith(".") and not code.startswith(".LBB"):
            continue
        funcs[cur].append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", code))
    return funcs


def parent_tree(rev, tmp):
    """csrc/ and include/ of `rev` unpacked under `tmp`"""
    tar = subprocess.run(["git", "-C", REPO, "archive", rev, CSRC, "include"], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
    return tmp


def default_parent(rev=None):
    """the revision to compare with: `rev` if given, else HEAD while csrc/ or include/ differ from it, else HEAD~1"""
    if rev is not None:
        return rev
    dirty = subprocess.run(["git", "-C", REPO, "status", "--porcelain", CSRC, "include"], capture_output=True, text=True).stdout
    return "HEAD" if dirty.strip() else "HEAD~1"


def differences(parent, name):
    """(functions in the parent, functions now, [what differs]) of csrc/<name> between the tree `parent` and this one"""
    asm_before, asm_after = assembly(parent, name), assembly(REPO, name)
    before, after = remarks(parent, name), remarks(REPO, name)
    figures = lambda k: {f: k[f] for f in FIELDS}
    diffs = [f"{name}: {f}: missing" for f in asm_before if f not in asm_after]
    diffs += [f"{name}: {f}: new" for f in asm_after if f not in asm_before]
    diffs += [f"{name}: {f}: instructions differ" for f in asm_before if f in asm_after and asm_before[f] != asm_after[f]]
    diffs += [f"{name}: {n}: resource figures differ" for n, k in before.items() if n in after and figures(k) != figures(after[n])]
    # the figures of every function named above that the compiler reports on, before -> after, with its instruction counts
    for n, k in before.items():
        sym = k["mangled"]
        if n in after and (figures(k) != figures(after[n]) or asm_before.get(sym) != asm_after.get(sym)):
            diffs.append(f"{name}: {n}: figures: instructions {len(asm_before.get(sym, []))} -> {len(asm_after.get(sym, []))}; "
                         + "; ".join(f"{f.split(' [')[0]} {k[f]} -> {after[n][f]}" for f in FIELDS))
    kernels = {k["mangled"] for k in before.values()}
    diffs += [f"{name}: {f}: figures: instructions {len(asm_before[f])} -> {len(asm_after[f])} (a device function: the compiler reports no figures of its own)"
              for f in asm_before if f in asm_after and asm_before[f] != asm_after[f] and f not in kernels]
    return len(asm_before), len(asm_after), diffs


def main():
    ap = argparse.ArgumentParser(description="compare the device code of csrc files with the parent commit's")
    ap.add_argument("files", nargs="+", help="files of csrc/, by name")
    ap.add_argument("--parent", default=None, metavar="REV")
    ap.add_argument("--allow-new", action="store_true", help="a device function the parent does not have is reported, not an error")
    args = ap.parse_args()
    rev = default_parent(args.parent)
    bad = []
    with tempfile.TemporaryDirectory() as tmp:
        parent = parent_tree(rev, tmp)
        for name in args.files:
            nb, na, diffs = differences(parent, os.path.basename(name))
            count = lambda what: sum(d.endswith(what) for d in diffs)
            print(f"{name}: {nb} device functions in {rev}, {na} now; missing {count(': missing')}, new {count(': new')}, "
                  f"instructions differ {count('instructions differ')}, resource figures differ {count('figures differ')}", flush=True)
            for d in diffs:
                print("  " + d)
            bad += [d for d in diffs if not (args.allow_new and d.endswith(": new")) and ": figures: " not in d]
    sys.exit(f"{len(bad)} differences from {rev}" if bad else 0)


if __name__ == "__main__":
    main()
