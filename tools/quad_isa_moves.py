"""Instructions of the quad rollout's step loop that only MOVE values (compiler ISA, product flags; no GPU needed).
usage: python tools/quad_isa_moves.py [kernel-substring] [extra hipcc flags ...]      (default: k_rollout_qILi1ELb0ELb0E)
Per basic block of the step loops (loop depth 2, program order; blocks of 20 instructions or more; GROUPS = 1 has one loop per
role wave, each announced by its header) and in total over the loops: all instructions, fp64 arithmetic, AGPR reads / writes,
64-bit and 32-bit vector moves, scalar moves (literal rebuilding), lane moves (spilled scalar registers), scalar loads, LDS
instructions, vector-memory instructions.  The four role waves are separate blocks: the block that holds the v_rndne_f64 of a
sin/cos is the trigonometry role (first half) or the psi role (after barrier B), the one with v_log_f32 / v_exp_f32 or v_ldexp_f64
the atmosphere role; the table roles are the blocks with the most LDS reads.  Registers, AGPRs and scratch of every k_rollout_q
instantiation come from the same compile (-Rpass-analysis=kernel-resource-usage)."""
import os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "f16_mpc_oop_py_amd", "csrc", "f16_dynamics.hip")
sub = sys.argv[1] if len(sys.argv) > 1 else "k_rollout_qILi1ELb0ELb0E"
with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, "dyn.s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast",
           "-DF16_FAST_TAN", "-DF16_FAST_POW", "-DF16_FAST_TRIG", "-DF16_FAST_DIV", "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", out, SRC] + sys.argv[2:]
    remarks = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    txt = open(out).read()

CL = ["all", "fp64", "agpr_rd", "agpr_wr", "vmov64", "vmov32", "smov", "lane", "sload", "lds", "vmem"]
FP64 = re.compile(r"v_(fma|fmac|mul|add|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|ldexp|frexp\w*|fract|floor|ceil|rndne|trunc)_f64")


def classes(op):
    c = ["all"]
    if FP64.match(op): c.append("fp64")
    if op.startswith("v_accvgpr_read"): c.append("agpr_rd")
    if op.startswith("v_accvgpr_write"): c.append("agpr_wr")
    if op.startswith(("v_mov_b64", "v_pk_mov_b32")): c.append("vmov64")
    if op.startswith("v_mov_b32"): c.append("vmov32")
    if op.startswith(("s_mov_b32", "s_mov_b64")): c.append("smov")
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")): c.append("lane")
    if op.startswith("s_load"): c.append("sload")
    if op.startswith("ds_"): c.append("lds")
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")): c.append("vmem")
    return c


MARK = (("v_rndne_f64", "sincos"), ("v_log_f32", "log"), ("v_exp_f32", "exp"), ("v_ldexp_f64", "ldexp"), ("s_barrier", "barrier"),
        ("global_store", "store"))
for m in re.finditer(r"\n(_Z\w+):[^\n]*\n", txt):
    if sub not in m.group(1) or m.group(1).endswith(".kd"):
        continue
    body = txt[m.end():]
    body = body[:body.find(".Lfunc_end")]
    print(m.group(1))
    tot = dict.fromkeys(CL, 0)
    for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body):
        own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", b[:400])     # (a header names its parent loop's depth first)
        d = own or re.search(r"Depth=(\d+)", b[:400])
        if not d or int(d.group(1)) < 2:                 # depth 1 is the loop over batches of 16 aircraft: prologue and epilogue
            continue
        if own:                                          # GROUPS = 1: one step loop per role wave, GROUPS = 2: one for all
            print(f"  step loop at {b.split(':')[0]}")
        ops = [l.split()[0] for l in b.split("\n")[1:] if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        c = dict.fromkeys(CL, 0)
        for op in ops:
            for k in classes(op): c[k] += 1
        for k in CL: tot[k] += c[k]
        if len(ops) >= 20:
            marks = ",".join(n for pat, n in MARK if any(op.startswith(pat) for op in ops))
            print(f"  {b.split(':')[0]:10s} " + " ".join(f"{k} {c[k]:4d}" for k in CL) + f"  [{marks}]")
    print("  step loop  " + " ".join(f"{k} {tot[k]:4d}" for k in CL))
name, res = None, {}
for l in remarks.split("\n"):
    f = re.search(r"Function Name: (\S+)", l)
    if f:
        q = re.search(r"k_rollout_qILi(\d)ELb(\d)ELb(\d)E", f.group(1))
        name = f"k_rollout_q<{q.group(1)},{q.group(2)},{q.group(3)}>" if q else None
    v = re.search(r" (VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", l)
    if name and v:
        res.setdefault(name, {})[v.group(1).split()[0]] = v.group(2)
for name, r in res.items():
    print(f"{name}: VGPRs {r.get('VGPRs')} AGPRs {r.get('AGPRs')} scratch {r.get('ScratchSize')} B/lane")
