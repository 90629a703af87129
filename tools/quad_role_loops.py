"""Structure of the quad rollout's step loops in the compiler's ISA (product flags; no GPU needed): one loop per role wave -- the
four roles of a step and the wave that stores the samples.
usage: python tools/quad_role_loops.py [--asm listing.s] [extra hipcc flags ...]
For every k_rollout_q instantiation, from the control-flow graph of its listing:
  (a) the role dispatch -- every conditional branch, outside the step loops, whose two sides lead to different step loops -- must be
      an s_cbranch_scc0/1 behind an s_cmp of the role index: a scalar branch.  A lane-masked dispatch (v_cmp, s_and_saveexec,
      s_cbranch_execz) would send a wave through another role's loop with an empty mask, and s_barrier does not look at the mask:
      the barrier counts of the four waves would come apart and the workgroup would hang.  Where the compiler joins two roles'
      paths and parts them again, it carries the outcome of the s_cmp in a scalar register pair and branches on `vcc = exec & pair`
      (or on EXEC itself, one way only): accepted while nothing in front of the branch writes EXEC, listed with the rest;
  (b) the number of s_barrier in each role's step loop, which must be the same in all five (two: A and B);
  (c) per step loop: instructions, branch instructions (every one a candidate for a taken jump), lane-mask (EXEC) operations, lane
      moves (v_readlane / v_writelane / v_readfirstlane: spilled scalar registers), scalar moves (literals rebuilt), with the totals
      of the single shared loop of the commit before beside them (PARENT, counted by this script on that commit's listing).
An instantiation that keeps ONE step loop (GROUPS = 2) has no dispatch; its loop is counted the same way.  Registers, AGPRs and
scratch of every instantiation come from the same compile.  Exit status 1 if (a) or (b) fails anywhere."""
import os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "f16_mpc_oop_py_amd", "csrc", "f16_dynamics.hip")
# the shared step loop of the commit before this tool (1e4ad57), same flags: all, branch, exec, lane, smov, barriers
PARENT = {"1,0,0": (1541, 54, 88, 44, 167, 2), "1,0,1": (1574, 56, 86, 34, 178, 2), "1,1,0": (1558, 52, 86, 48, 169, 2),
          "1,1,1": (1608, 56, 86, 60, 168, 2)}
PARENT_RES = {"1,0,0": (254, 0, 0), "2,0,0": (256, 0, 64), "1,0,1": (254, 0, 0), "2,0,1": (256, 0, 48), "1,1,0": (255, 16, 0),
              "2,1,0": (256, 0, 136), "1,1,1": (255, 14, 0), "2,1,1": (256, 0, 128)}       # VGPRs, AGPRs, scratch bytes per lane

args = sys.argv[1:]
remarks = ""
if args[:1] == ["--asm"]:
    txt = open(args[1]).read()
else:
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dyn.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast",
               "-DF16_FAST_TAN", "-DF16_FAST_POW", "-DF16_FAST_TRIG", "-DF16_FAST_DIV", "-S", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-o", out, SRC] + args
        remarks = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
        txt = open(out).read()

CL = ["all", "branch", "exec", "lane", "smov", "barrier"]
EXEC = re.compile(r"s_\w+_saveexec_b64|s_(or|and|andn2|xor|mov)_b64 exec\b")


def classes(line):
    op = line.split()[0]
    c = ["all"]
    if op.startswith(("s_branch", "s_cbranch")): c.append("branch")
    if EXEC.match(line): c.append("exec")
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")): c.append("lane")
    if op.startswith(("s_mov_b32", "s_mov_b64")) and not EXEC.match(line): c.append("smov")
    if op == "s_barrier": c.append("barrier")
    return c


class Block:
    def __init__(self, name, head):
        self.name, self.ins, self.succ = name, [], []
        h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", head)
        own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", head)
        self.loop = name if own else (h.group(1) if h else None)           # innermost loop
        self.depth = int(own.group(1)) if own else (int(h.group(2)) if h else 0)


def blocks_of(body):
    """basic blocks in program order; labelled ones by label, fall-through ones as %bb.N"""
    out, cur, lines = [], None, body.split("\n")
    for i, l in enumerate(lines):
        m = re.match(r"(?:\.L(BB\d+_\d+):|; %(bb\.\d+):)(.*)", l)
        if m:
            head, j = m.group(3), i + 1
            while j < len(lines) and re.match(r"\s+;", lines[j]):      # (a loop header's comment runs over several lines)
                head, j = head + lines[j], j + 1
            cur = Block(m.group(1) or m.group(2), head)
            out.append(cur)
        elif cur is not None and l.startswith("\t") and not l.strip().startswith((".", ";")):
            cur.ins.append(re.sub(r"\s*;.*$", "", l.strip()))
    for i, b in enumerate(out):
        last = b.ins[-1].split()[0] if b.ins else ""
        for ins in b.ins:
            t = re.match(r"s_c?branch\w*\s+\.L(BB\d+_\d+)", ins)
            if t: b.succ.append(t.group(1))
        if last not in ("s_branch", "s_endpgm") and i + 1 < len(out):
            b.succ.append(out[i + 1].name)
    return out


def count(bl):
    c = dict.fromkeys(CL, 0)
    for b in bl:
        for ins in b.ins:
            for k in classes(ins): c[k] += 1
    return c


def row(c):
    return " ".join(f"{k} {c[k]:4d}" for k in CL)


ok = True
for m in re.finditer(r"\n(_ZN3f1611k_rollout_qILi(\d)ELb(\d)ELb(\d)E\w*):[^\n]*\n", txt):
    key = ",".join(m.group(2, 3, 4))
    body = txt[m.end():]
    body = body[:body.find(".Lfunc_end")]
    bl = blocks_of(body)
    by = {b.name: b for b in bl}
    heads = [b.name for b in bl if b.loop == b.name and b.depth == 2]
    loops = {h: [b for b in bl if b.loop == h] for h in heads}
    outer = [b.name for b in bl if b.loop == b.name and b.depth == 1 and any(x.depth == 2 for x in bl)]
    print(f"k_rollout_q<{key}>: {len(heads)} step loop{'s' if len(heads) != 1 else ''}")
    # which step loops a block leads to within one pass of the batch loop (no edge back to a depth-1 header)
    reach = {b.name: ({b.loop} if b.loop in loops else set()) for b in bl}
    changed = True
    while changed:
        changed = False
        for b in bl:
            if b.loop in loops: continue
            r = set(reach[b.name])
            for s in b.succ:
                if s in by and s not in outer: r |= reach[s]
            if r != reach[b.name]: reach[b.name], changed = r, True
    if len(heads) == 5:
        nscalar = 0
        for bi, b in enumerate(bl):
            if b.loop in loops: continue
            for i, ins in enumerate(b.ins):
                t = re.match(r"(s_cbranch\w*)\s+\.L(BB\d+_\d+)", ins)
                if not t: continue
                # the other side: every later branch target of the block and its fall-through
                rest = [x.group(1) for x in (re.match(r"s_c?branch\w*\s+\.L(BB\d+_\d+)", y) for y in b.ins[i + 1:]) if x]
                if b.ins[-1].split()[0] != "s_branch" and bi + 1 < len(bl): rest.append(bl[bi + 1].name)
                other = set().union(*[reach.get(x, set()) for x in rest]) if rest else set()
                taken = reach.get(t.group(2), set())
                if not taken or not other or taken == other: continue          # (a guard round one loop, or no choice between loops)
                before = b.ins[:i]
                masked = any(EXEC.match(x) and "saveexec" in x for x in before)
                if t.group(1) in ("s_cbranch_scc0", "s_cbranch_scc1"):
                    setter = next((x for x in reversed(before) if re.match(r"s_(cmp|bitcmp|and|or|andn2|xor|add|sub|lshl|lshr|bfe)", x)), "?")
                    good, what = setter.startswith("s_cmp") and not masked, "scalar compare and branch"
                    nscalar += good
                elif t.group(1) in ("s_cbranch_vccz", "s_cbranch_vccnz"):
                    setter = next((x for x in reversed(before) if re.match(r"\w+\s+vcc\b", x)), "?")
                    good = bool(re.match(r"s_(and|andn2)_b64 vcc, exec, s\[", setter)) and not masked
                    what = "a wave-uniform flag in a scalar register pair, EXEC not written"
                else:
                    setter = "-"
                    good, what = not any(EXEC.match(x) for x in before), "on EXEC, which this block does not write: one way only"
                ok &= good
                print(f"  (a) {b.name:9s} {setter}  ->  {ins}   {what if good else 'LANE-MASKED OR NOT A SCALAR CONDITION'}")
        if nscalar < 2:
            ok = False
            print("  (a) fewer than two scalar compares of the role index found")
        counts = [count(loops[h]) for h in heads]
        same = len({c["barrier"] for c in counts}) == 1 and counts[0]["barrier"] > 0
        ok &= same
        print(f"  (b) s_barrier per step loop: {[c['barrier'] for c in counts]}  {'equal' if same else 'NOT EQUAL'}")
        for h, c in zip(heads, counts):
            ops = [i.split()[0] for b in loops[h] for i in b.ins]
            # marks as in tools/quad_resident_isa.py (role_of): the store wave has the sample's stores and no fp64 arithmetic, the
            # table waves clamp a breakpoint guess and form table addresses
            role = ("atmosphere/actuators (wave 3)" if any(o.startswith(("v_log_f32", "v_exp_f32", "v_ldexp_f64")) for o in ops) else
                    "sample stores (wave 4)" if any(o.startswith("global_store") for o in ops) and not any(re.match(r"v_\w+_f64", o) and not o.startswith("v_cmp") for o in ops) else
                    "trigonometry/forces (wave 2)" if not any(o.startswith(("v_max_i32", "v_mad_u64_u32")) for o in ops) else
                    "longitudinal tables + psi (wave 0)" if any(o.startswith("v_rndne_f64") for o in ops) else "lateral tables/moments (wave 1)")
            pre = count([b for b in bl if b.loop not in loops and reach[b.name] == {h}])
            print(f"  (c) {h:9s} {row(c)}  [{role}; its first trip apart, outside the loop: {pre['all']} instructions, {pre['barrier']} s_barrier]")
        if key in PARENT:
            print("      before    " + row(dict(zip(CL, PARENT[key]))) + "  [one loop, every role wave walks all of it]")
    elif len(heads) == 1:
        c = count(loops[heads[0]])
        good = c["barrier"] == 2
        ok &= good
        print("  (a) one shared step loop: no role dispatch")
        print(f"  (b) s_barrier in the step loop: {c['barrier']}  {'(A and B)' if good else 'NOT TWO'}")
        print(f"  (c) {heads[0]:9s} {row(c)}  [all four roles]")
    else:
        ok = False
        print("  NEITHER ONE STEP LOOP NOR FIVE")
name, res = None, {}
for l in remarks.split("\n"):
    f = re.search(r"Function Name: (\S+)", l)
    if f:
        q = re.search(r"k_rollout_qILi(\d)ELb(\d)ELb(\d)E", f.group(1))
        name = ",".join(q.group(1, 2, 3)) if q else None
    v = re.search(r" (VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", l)
    if name and v:
        res.setdefault(name, {})[v.group(1).split()[0]] = int(v.group(2))
for name, r in res.items():
    p = PARENT_RES.get(name)
    print(f"k_rollout_q<{name}>: VGPRs {r.get('VGPRs')} AGPRs {r.get('AGPRs')} scratch {r.get('ScratchSize')} B/lane"
          + (f"   (before: VGPRs {p[0]} AGPRs {p[1]} scratch {p[2]} B/lane)" if p else ""))
print("PASS" if ok else "FAIL")
sys.exit(0 if ok else 1)
