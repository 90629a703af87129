"""What carrying the table corners across steps changes in the compiler's ISA of f16_dynamics.hip (product flags; no GPU needed).
usage: python tools/quad_corner_isa.py PARENT_TREE [HEAD_TREE]       (trees: checkouts of the two commits; HEAD_TREE defaults to this one)
   or: python tools/quad_corner_isa.py --asm parent.s parent.remarks head.s head.remarks      (listings + stderr of
       hipcc ... -S --cuda-device-only -Rpass-analysis=kernel-resource-usage, the flags of tools/quad_role_loops.py)
Prints
  (1) every function of the file compared between the two listings (comments and debug directives dropped): which ones differ;
  (2) VGPRs, AGPRs and scratch of every k_rollout_q instantiation, before and after;
  (3) for the two table loops (wave 0: the loop with the psi sin/cos, wave 1: the other loop that reads breakpoints) of every
      k_rollout_q<1,*>: instructions, VALU instructions, LDS reads by kind, 64-bit integer multiply-adds (address arithmetic),
      AGPR moves and scratch accesses (these two for the whole loop as well) ON THE HIT PATH -- the blocks a trip walks when every lane is still in last step's cell.
      The hit path is read off the control-flow graph: the blocks that lie on a way from the loop header back to it which avoids
      the block holding the breakpoint reads of the full lookup (the block of the loop that ends in an `s_branch`, reads LDS at
      least four times and hands the cell indices round the quad: six `v_mov_b32_dpp` or more).  `s_cbranch_execnz` in a block that does not write
      EXEC is how the compiler spells an unconditional jump and is followed as one."""
import os, re, subprocess, sys, tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-DF16_FAST_TAN", "-DF16_FAST_POW",
         "-DF16_FAST_TRIG", "-DF16_FAST_DIV", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
HERE = os.path.dirname(os.path.abspath(__file__))


def listing(tree):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dyn.s")
        src = os.path.join(tree, "f16_mpc_oop_py_amd", "csrc", "f16_dynamics.hip")
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-o", out, src], check=True, stderr=subprocess.PIPE, text=True)
        return open(out).read(), r.stderr


def functions(txt):
    """name -> instruction and label lines, comments and directives dropped"""
    out = {}
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n", txt):
        if f".type\t{m.group(1)},@function" not in txt: continue          # (data objects have labels of the same form)
        body = txt[m.end():]
        body = body[:body.find(".Lfunc_end")]
        keep = []
        for l in body.split("\n"):
            l = re.sub(r"\s*;.*$", "", l).rstrip()
            if not l or l.lstrip().startswith("."):
                if re.match(r"\.LBB\d+_\d+:", l): keep.append(l)
                continue
            keep.append(l.strip())
        out[m.group(1)] = keep
    return out


def resources(remarks):
    name, res = None, {}
    for l in remarks.split("\n"):
        f = re.search(r"Function Name: (\S+)", l)
        if f:
            q = re.search(r"k_rollout_qILi(\d)ELb(\d)ELb(\d)E", f.group(1))
            name = ",".join(q.group(1, 2, 3)) if q else None
        v = re.search(r" (VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", l)
        if name and v: res.setdefault(name, {})[v.group(1).split()[0]] = int(v.group(2))
    return res


def loops(txt, fname):
    """step loops (depth 2) of one function: header -> list of (block name, instructions, successors)"""
    m = next(m for m in re.finditer(r"\n(_Z\w+):[^\n]*\n", txt) if m.group(1) == fname)
    body = txt[m.end():]
    body = body[:body.find(".Lfunc_end")]
    bl, cur, lines = [], None, body.split("\n")
    for i, l in enumerate(lines):
        mm = re.match(r"(?:\.L(BB\d+_\d+):|; %(bb\.\d+):)(.*)", l)
        if mm:
            head, j = mm.group(3), i + 1
            while j < len(lines) and re.match(r"\s+;", lines[j]): head, j = head + lines[j], j + 1
            own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", head)
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", head)
            name = mm.group(1) or mm.group(2)
            cur = {"name": name, "ins": [], "loop": name if own else (h.group(1) if h else None),
                   "depth": int(own.group(1)) if own else (int(h.group(2)) if h else 0)}
            bl.append(cur)
        elif cur is not None and l.startswith("\t") and not l.strip().startswith((".", ";")):
            cur["ins"].append(re.sub(r"\s*;.*$", "", l.strip()))
    for i, b in enumerate(bl):
        b["succ"] = []
        uncond = False
        for ins in b["ins"]:
            t = re.match(r"(s_c?branch\w*)\s+\.L(BB\d+_\d+)", ins)
            if not t: continue
            b["succ"].append(t.group(2))
            if t.group(1) == "s_branch" or (t.group(1) == "s_cbranch_execnz" and not any(len(x.split()) > 1 and x.split()[1].startswith("exec") for x in b["ins"])):
                uncond = True
        if not uncond and i + 1 < len(bl): b["succ"].append(bl[i + 1]["name"])
    heads = [b["name"] for b in bl if b["loop"] == b["name"] and b["depth"] == 2]
    return {h: [b for b in bl if b["loop"] == h] for h in heads}


def hit_path(blocks, header):
    by = {b["name"]: b for b in blocks}
    full = [b for b in blocks if b["ins"] and b["ins"][-1].startswith("s_branch")
            and sum(i.startswith("ds_read") for i in b["ins"]) >= 4 and sum(i.startswith("v_mov_b32_dpp") for i in b["ins"]) >= 6]
    if len(full) != 1: return None
    gone = full[0]["name"]
    fwd, stack = set(), [header]
    while stack:
        n = stack.pop()
        if n in fwd or n == gone or n not in by: continue
        fwd.add(n)
        stack += [s for s in by[n]["succ"] if s != header]
    back = {b["name"] for b in blocks if header in b["succ"] and b["name"] != gone}
    changed = True
    while changed:
        changed = False
        for b in blocks:
            if b["name"] not in back and b["name"] != gone and any(s in back for s in b["succ"]):
                back.add(b["name"]); changed = True
    return [b for b in blocks if b["name"] in fwd and b["name"] in back]


def count(blocks):
    ops = [i.split()[0] for b in blocks for i in b["ins"]]
    c = {"instructions": len(ops), "VALU": sum(o.startswith("v_") for o in ops),
         "ds_read2_b64": sum(o == "ds_read2_b64" for o in ops), "ds_read_b64": sum(o == "ds_read_b64" for o in ops),
         "other LDS reads": sum(o.startswith("ds_read") and o not in ("ds_read2_b64", "ds_read_b64") for o in ops),
         "v_mad_u64_u32": sum(o.startswith("v_mad_u64_u32") for o in ops), "v_accvgpr_*": sum(o.startswith("v_accvgpr") for o in ops),
         "scratch_*": sum(o.startswith("scratch_") for o in ops), "s_barrier": ops.count("s_barrier")}
    return c


def table_loops(txt, fname):
    out = {}
    for h, blocks in loops(txt, fname).items():
        ops = [i.split()[0] for b in blocks for i in b["ins"]]
        if any(o.startswith(("v_log_f32", "v_exp_f32", "v_ldexp_f64", "global_store")) for o in ops): continue     # waves 3 and 2
        role = "wave 0" if any(o.startswith("v_rndne_f64") for o in ops) else "wave 1"
        hp = hit_path(blocks, h)
        out[role] = (h, count(blocks), count(hp) if hp is not None else None)
    return out


a = sys.argv[1:]
if a[:1] == ["--asm"]:
    (pt, pr), (ht, hr) = [(open(a[i]).read(), open(a[i + 1]).read()) for i in (1, 3)]
else:
    pt, pr = listing(a[0])
    ht, hr = listing(a[1] if len(a) > 1 else os.path.join(HERE, ".."))

pf, hf = functions(pt), functions(ht)
diff = [n for n in pf if n in hf and pf[n] != hf[n]]
only = sorted(set(pf) ^ set(hf))
print(f"(1) functions: {len(pf)} before, {len(hf)} after; {len(pf) - len(diff) - len([n for n in only if n in pf])} identical instruction for instruction")
for n in diff:
    print(f"    differs: {n[:70]}  ({len(pf[n])} -> {len(hf[n])} lines)")
for n in only:
    print(f"    only {'before' if n in pf else 'after'}: {n[:70]}")
print("(2) registers: VGPRs + AGPRs, scratch bytes per lane")
rp, rh = resources(pr), resources(hr)
for k in rh:
    p, h = rp.get(k, {}), rh[k]
    print(f"    k_rollout_q<{k}>: {p.get('VGPRs')} + {p.get('AGPRs')}, {p.get('ScratchSize')} B  ->  {h['VGPRs']} + {h['AGPRs']}, {h['ScratchSize']} B")
print("(3) table loops of k_rollout_q<1,*>: whole loop and hit path, before -> after")
for n in hf:
    q = re.match(r"_ZN3f1611k_rollout_qILi1ELb(\d)ELb(\d)E", n)
    if not q or n not in pf: continue
    tp, th = table_loops(pt, n), table_loops(ht, n)
    for role in ("wave 0", "wave 1"):
        (_, wp, hp), (_, wh, hh) = tp[role], th[role]
        print(f"    <1,{q.group(1)},{q.group(2)}> {role}: loop {wp['instructions']} -> {wh['instructions']} instructions; in the whole loop "
              f"v_accvgpr_* {wp['v_accvgpr_*']} -> {wh['v_accvgpr_*']}, scratch_* {wp['scratch_*']} -> {wh['scratch_*']}")
        if hp is None or hh is None:
            print("      hit path not identified")
            continue
        for k in hp:
            print(f"      hit path {k:16s} {hp[k]:4d} -> {hh[k]:4d}")
