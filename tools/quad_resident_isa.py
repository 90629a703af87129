"""The role loops of every k_rollout_q<1,*> in the compiler's ISA -- the four roles of a step and the wave that stores the samples:
what a step still loads, moves and publishes (no GPU needed).
usage: python tools/quad_resident_isa.py PARENT_TREE [HEAD_TREE]     (checkouts of the two commits; HEAD_TREE defaults to this one)
   or: python tools/quad_resident_isa.py --asm parent.s parent.remarks head.s head.remarks     (listings + stderr of
       hipcc ... -S --cuda-device-only -Rpass-analysis=kernel-resource-usage, the flags of tools/quad_role_loops.py)
   or: python tools/quad_resident_isa.py --so f16_mpc_oop_py_amd/libf16hip.so       (the BUILT library: its gfx950 code object is
       unbundled and disassembled; prints, per role loop, scalar loads and s_barrier only -- what tests/test_quad_resident_isa.py
       reads: sixteen `wave N` lines for the four roles of a step; the store wave's loop is reported on a line of another form and
       gated the same way: one loop, no scalar load, two barriers, no fp64 arithmetic)
Two listings: prints
  (1) every function of the file compared between the two (comments and directives dropped): which ones differ;
  (2) VGPRs, AGPRs, scratch of every k_rollout_q instantiation;
  (3) per role loop of every <1,*> instantiation, before -> after: instructions, scalar loads, lane moves (v_readlane / v_writelane /
      v_readfirstlane), v_accvgpr_*, 64-bit vector moves, scratch accesses, s_barrier, fp64 arithmetic instructions, and whether
      the fp64 EXPRESSION TREES of the loop agree: every fp64 arithmetic instruction is evaluated symbolically over the loop's
      blocks in program order (operands: the tree that last wrote the register pair, followed through vector moves; a scalar
      register, a value loaded or produced by any other instruction, or a register written outside the loop is an anonymous leaf;
      inline constants and operand modifiers -- neg, abs, clamp, omod -- are part of the node) and the multisets of trees compared;
      LDS reads per loop are listed with the counts;
  (4) wave 2: ds_write* between its last fp64 instruction of the second half and barrier A.
  (5) the store wave's loop of the head (the parent may have none): one per instantiation, no scalar load, two s_barrier, no fp64
      arithmetic, its global stores.
Exit status 1 if the gate fails: a scalar load in a role loop of the head; more lane moves, v_accvgpr_*, 64-bit moves or scratch
in a loop than before; scratch in a <1,*> instantiation; fp64 trees that differ in any of the four loops of a step; more than
three ds_write* in (4); barriers other than two per loop; a store loop that fails (5); any function outside k_rollout_q<1,*> that
differs.
A canonicalisation, `v_max_f64 d, x, x`, is the identity on every value but a signalling NaN: the evaluator follows it like a move
(of a leaf it makes a leaf) and it is no tree of its own; they are counted apart.  Where the compiler hoists one out of a loop or
leaves it inside, the trees stay the same.
Differences a change has BY DESIGN are named on the command line, never in this file (default: none, and then every gate above is
the strict one):
  --named ROLE:SIDE:TREE   one tree that only SIDE (before | after) has in the loop of ROLE (0..3), in the form the tool prints for
                           unmatched trees, e.g. `v_mul_f64(L;v_add_f64(L;neg L))` (a trailing `...`: any tree that starts so);
                           taken out of the comparison once per
                           instantiation, and it is an error if it is not there.  What is left must be identical.
  --more INST:ROLE:KEY:N   the loop of ROLE in instantiation INST (`1,0,0` ...; `*`: all) may have N more `lane moves` or
                           `64-bit moves` than before.
The record of a change (profiles/*_isa.txt) starts with the command line that made it."""
import collections, hashlib, os, re, subprocess, sys, tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-DF16_FAST_TAN", "-DF16_FAST_POW",
         "-DF16_FAST_TRIG", "-DF16_FAST_DIV", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
HERE = os.path.dirname(os.path.abspath(__file__))
LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))), "llvm", "bin")
FP64 = re.compile(r"v_(fma|fmac|mul|add|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|ldexp|frexp\w*|fract|floor|ceil|rndne|trunc)_f64")
ROLES = ["wave 0 longitudinal tables, psi", "wave 1 lateral tables, moments", "wave 2 trigonometry, forces", "wave 3 atmosphere, actuators",
         "wave 4 sample stores"]
NAMES = {}          # tree -> the instruction at its root (for the listing of unmatched trees)
KEYS = ["instructions", "LDS reads", "s_load", "lane moves", "v_accvgpr", "64-bit moves", "scratch", "s_barrier", "fp64", "canonicalisations"]
EXPR = {}           # tree -> its readable form


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
        if f".type\t{m.group(1)},@function" not in txt: continue
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


def blocks_of_listing(txt, fname):
    m = next(m for m in re.finditer(r"\n(_Z\w+):[^\n]*\n", txt) if m.group(1) == fname)
    body = txt[m.end():]
    body = body[:body.find(".Lfunc_end")]
    bl, cur = [], {"name": "entry", "ins": []}
    bl.append(cur)
    for l in body.split("\n"):
        mm = re.match(r"\.L(BB\d+_\d+):", l)
        if mm:
            cur = {"name": mm.group(1), "ins": []}
            bl.append(cur)
        elif l.startswith("\t") and not l.strip().startswith((".", ";")):
            if cur["ins"] and re.match(r"s_c?branch", cur["ins"][-1]):             # (a block ends with its branch)
                cur = {"name": f"{cur['name']}+", "ins": []}
                bl.append(cur)
            cur["ins"].append(re.sub(r"\s*;.*$", "", l.strip()))
    for b in bl:
        b["targets"] = [t.group(1) for t in (re.match(r"s_c?branch\w*\s+\.L(BB\d+_\d+)", i) for i in b["ins"]) if t]
    return bl


def code_object_functions(so):
    """name -> blocks, from the disassembly of the gfx950 code object bundled in a built library"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fat}", f"--output={co}"], check=True)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, stdout=subprocess.PIPE, text=True).stdout
    out, cur = {}, None
    for l in dis.split("\n"):
        f = re.match(r"[0-9a-f]+ <(\S+)>:", l)
        if f:
            cur = out.setdefault(f.group(1), [])
            continue
        m = re.match(r"\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", l)
        if cur is not None and m: cur.append((int(m.group(2), 16), m.group(1)))
    fns = {}
    for name, ins in out.items():
        if "k_rollout_q" not in name: continue
        tg = {}
        for i, (addr, txt) in enumerate(ins):
            t = re.match(r"s_c?branch\w*\s+(-?\d+)", txt)
            if t:
                simm = int(t.group(1)) & 0xFFFF
                tg[i] = addr + 4 + 4 * (simm - 0x10000 if simm & 0x8000 else simm)
        starts = {ins[0][0]} | set(tg.values()) | {ins[i + 1][0] for i in tg if i + 1 < len(ins)}
        bl, cur_b = [], None
        for i, (addr, txt) in enumerate(ins):
            if addr in starts:
                cur_b = {"name": f"{addr:x}", "ins": [], "targets": []}
                bl.append(cur_b)
            cur_b["ins"].append(txt)
            if i in tg: cur_b["targets"].append(f"{tg[i]:x}")
        fns[name] = bl
    return fns


def step_loops(bl):
    """the step loops: the strongly connected parts of the batch loop once its header is taken out, that hold an s_barrier"""
    for i, b in enumerate(bl):
        last = b["ins"][-1].split()[0] if b["ins"] else ""
        b["succ"] = list(b["targets"]) + ([bl[i + 1]["name"]] if last not in ("s_branch", "s_endpgm") and i + 1 < len(bl) else [])

    def sccs(names):
        by = {b["name"]: b for b in bl if b["name"] in names}
        idx, low, st, on, out, n = {}, {}, [], set(), [], [0]
        for root in by:
            if root in idx: continue
            work = [(root, iter(by[root]["succ"]))]
            idx[root] = low[root] = n[0]; n[0] += 1; st.append(root); on.add(root)
            while work:
                v, it = work[-1]
                adv = False
                for w in it:
                    if w not in by: continue
                    if w not in idx:
                        idx[w] = low[w] = n[0]; n[0] += 1; st.append(w); on.add(w)
                        work.append((w, iter(by[w]["succ"])))
                        adv = True
                        break
                    if w in on: low[v] = min(low[v], idx[w])
                if adv: continue
                work.pop()
                if work: low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == idx[v]:
                    comp = set()
                    while True:
                        w = st.pop(); on.discard(w); comp.add(w)
                        if w == v: break
                    if len(comp) > 1 or v in by[v]["succ"]: out.append(comp)
        return out
    has_bar = lambda comp: any(i == "s_barrier" for b in bl if b["name"] in comp for i in b["ins"])
    top = [c for c in sccs({b["name"] for b in bl}) if has_bar(c)]
    loops = []
    for c in top:
        inner = []
        # the batch loop's header: the block of the part that is entered from outside it
        heads = [b["name"] for b in bl if b["name"] in c and any(b["name"] in p["succ"] for p in bl if p["name"] not in c)]
        sub = sccs(c - set(heads[:1])) if heads else []
        inner = [s for s in sub if has_bar(s)]
        loops += inner if inner else [c]
    return [[b for b in bl if b["name"] in c] for c in loops]


def role_of(blocks):
    ops = [i.split()[0] for b in blocks for i in b["ins"]]
    if any(o.startswith(("v_log_f32", "v_exp_f32", "v_ldexp_f64")) for o in ops): return 3
    # the store wave: the sample's stores and no fp64 arithmetic at all (before it existed the stores stood in wave 2's loop)
    if any(o.startswith("global_store") for o in ops) and not any(FP64.match(o) for o in ops): return 4
    # the table waves clamp a breakpoint guess and form table addresses (their miss path); wave 2 does neither
    if not any(o.startswith(("v_max_i32", "v_mad_u64_u32")) for o in ops): return 2
    return 0 if any(o.startswith("v_rndne_f64") for o in ops) else 1


def canonicalisation(ins):
    m = re.match(r"v_max_f64\S*\s+\S+,\s*(\S+),\s*(\S+)$", ins)
    return bool(m) and m.group(1) == m.group(2)


def count(blocks):
    ops = [i.split()[0] for b in blocks for i in b["ins"]]
    canon = sum(canonicalisation(i) for b in blocks for i in b["ins"])
    return {"canonicalisations": canon, "global stores": sum(o.startswith("global_store") for o in ops),"instructions": len(ops), "LDS reads": sum(o.startswith("ds_read") for o in ops), "s_load": sum(o.startswith(("s_load", "s_buffer_load")) for o in ops),
            "lane moves": sum(o.startswith(("v_readlane", "v_writelane", "v_readfirstlane")) for o in ops),
            "v_accvgpr": sum(o.startswith("v_accvgpr") for o in ops), "64-bit moves": sum(o.startswith(("v_mov_b64", "v_pk_mov_b32")) for o in ops),
            "scratch": sum(o.startswith("scratch_") for o in ops), "s_barrier": ops.count("s_barrier"), "fp64": sum(bool(FP64.match(o)) for o in ops) - canon}


def regs(tok):
    """vector registers of an operand token, as a list of 32-bit register numbers (None: not a vector register)"""
    t = re.sub(r"^(-|\|)+|\|$", "", tok)
    m = re.fullmatch(r"([va])(\d+)", t)
    if m: return [m.group(1) + m.group(2)]
    m = re.fullmatch(r"([va])\[(\d+):(\d+)\]", t)
    if m: return [m.group(1) + str(k) for k in range(int(m.group(2)), int(m.group(3)) + 1)]
    return None


def trees(blocks):
    """multiset of the symbolic trees of the fp64 arithmetic instructions of a loop (see the module text)"""
    val, out = {}, collections.Counter()
    h = lambda s: hashlib.sha1(s.encode()).hexdigest()[:16]

    def operand(tok):
        r = regs(tok)
        mod = ("neg " if tok.startswith("-") else "") + ("abs " if "|" in tok else "")
        if r is None:
            return mod + ("L" if re.match(r"-?\|?(s\d|s\[|vcc|exec|ttmp)", tok) else tok)
        parts = [val.get(x) for x in r]
        if parts[0] is not None and all(p is not None and p[0] == parts[0][0] and p[1] == k for k, p in enumerate(parts)):
            return mod + parts[0][0]
        return mod + "L"
    for b in blocks:
        for ins in b["ins"]:
            op, _, rest = ins.partition(" ")
            toks = [t.strip() for t in rest.split(",")] if rest.strip() else []
            if not toks: continue
            flags = toks[-1].split()[1:] if " " in toks[-1] else []
            toks[-1] = toks[-1].split()[0]
            dst = regs(toks[0])
            if canonicalisation(ins) and dst:
                # the identity: the tree of the source (a leaf stays a leaf; a negated tree is a node of its own, not counted)
                t = operand(toks[1])
                if t.split(" ")[-1] == "L":
                    for x in dst: val.pop(x, None)
                else:
                    e = t if re.fullmatch(r"[0-9a-f]{16}", t) else h("canon(" + t + ")")
                    if e not in EXPR: EXPR[e] = "canon(" + " ".join(EXPR.get(w, w) for w in t.split(" ")) + ")"
                    for k, x in enumerate(dst): val[x] = (e, k)
                continue
            if FP64.match(op):
                src = toks[1:]
                if op.startswith("v_div_scale"): src = toks[2:]                 # (a second, scalar destination)
                args = [operand(t) for t in src]
                if op.startswith("v_fmac_f64"): args.append(operand(toks[0]))
                name = "v_fma_f64" if op.startswith("v_fmac_f64") else re.sub(r"_e(32|64)$", "", op)
                if name in ("v_fma_f64", "v_mul_f64", "v_add_f64", "v_max_f64", "v_min_f64"):    # commutative in the first two
                    args[:2] = sorted(args[:2])
                e = h(name + "(" + ";".join(args) + ")" + " ".join(sorted(flags)))
                out[e] += 1
                NAMES[e] = name
                EXPR[e] = name + "(" + ";".join(" ".join(EXPR.get(w, w) for w in x.split(" ")) for x in args) + ")" + "".join(" " + f for f in sorted(flags))
                if dst:
                    for k, x in enumerate(dst): val[x] = (e, k)
            elif dst is not None:
                srcr = regs(toks[1]) if len(toks) > 1 else None
                if op.split("_e")[0] in ("v_mov_b32", "v_mov_b64", "v_pk_mov_b32", "v_accvgpr_read_b32", "v_accvgpr_write_b32", "v_accvgpr_mov_b32") \
                        and srcr is not None and len(srcr) >= len(dst) and "dpp" not in ins and "sdwa" not in ins and not flags:
                    for k, x in enumerate(dst): val[x] = val.get(srcr[k] if op != "v_pk_mov_b32" or k == 0 else regs(toks[2])[1])
                elif not op.startswith(("ds_write", "global_store", "scratch_store", "flat_store")):     # (their first operand is an address)
                    for x in dst: val.pop(x, None)
    return out


def publish_writes(blocks):
    """wave 2: the most ds_write* on any way through the loop from an fp64 instruction to barrier A that passes no further fp64
    instruction and no other barrier -- what stands between the last Euler update and barrier A.  Barrier A is the s_barrier from
    which the sin/cos (v_rndne_f64, first half) is reached without passing the other one.  Ways, not program order: the compiler
    places the blocks of a half as it likes."""
    by = {b["name"]: b for b in blocks}
    nodes = [(b["name"], k) for b in blocks for k in range(len(b["ins"]))]
    ins = {n: by[n[0]]["ins"][n[1]] for n in nodes}

    def succ(n):
        b = by[n[0]]
        if n[1] + 1 < len(b["ins"]): return [(n[0], n[1] + 1)]
        return [(s, 0) for s in b["succ"] if s in by and by[s]["ins"]]
    bars = [n for n in nodes if ins[n] == "s_barrier"]
    if len(bars) != 2: return None

    def reaches_sincos(bar):
        seen, stack = set(), succ(bar)
        while stack:
            n = stack.pop()
            if n in seen or ins[n] == "s_barrier": continue
            seen.add(n)
            if ins[n].startswith("v_rndne_f64"): return True
            stack += succ(n)
        return False
    A = [b for b in bars if reaches_sincos(b)]
    if len(A) != 1: return None
    memo = {}

    def best(n):            # most ds_write* from behind n to barrier A on fp64-free, barrier-free ways; None: no such way
        if n in memo: return memo[n]
        memo[n] = None          # (a cycle without a barrier does not count)
        r = None
        for m in succ(n):
            if m == A[0]: v = 0
            elif ins[m] == "s_barrier" or FP64.match(ins[m]): continue
            else:
                v = best(m)
                if v is None: continue
                v += ins[m].startswith("ds_write")
            r = v if r is None else max(r, v)
        memo[n] = r
        return r
    sys.setrecursionlimit(20000)
    found = [best(n) for n in nodes if FP64.match(ins[n])]
    found = [v for v in found if v is not None]
    return max(found) if found else None


def role_loops(bl):
    out = {}
    for blocks in step_loops(bl):
        out.setdefault(role_of(blocks), []).append(blocks)
    return out


a = sys.argv[1:]
NAMED_TREES, MORE = [], {}
while "--named" in a or "--more" in a:
    i = min(a.index(x) for x in ("--named", "--more") if x in a)
    if a[i] == "--named":
        role, side, expr = a[i + 1].split(":", 2)
        assert side in ("before", "after"), side
        NAMED_TREES.append((int(role), side, expr))
    else:
        inst, role, key, n = a[i + 1].split(":")
        MORE[(inst, int(role), key)] = int(n)
    del a[i:i + 2]
more = lambda inst, r, k: MORE.get((inst, r, k), MORE.get(("*", r, k), 0))
if a[:1] == ["--so"]:
    ok = True
    fns = code_object_functions(a[1])
    names = sorted(n for n in fns if re.match(r"_ZN3f1611k_rollout_qILi1ELb\dELb\dE", n))
    if len(names) != 4:
        print(f"expected four k_rollout_q<1,*> in the code object, found {len(names)}"); ok = False
    for n in names:
        q = re.match(r"_ZN3f1611k_rollout_qILi1ELb(\d)ELb(\d)E", n)
        rl = role_loops(fns[n])
        if sorted(rl) != [0, 1, 2, 3, 4] or any(len(v) != 1 for v in rl.values()):
            print(f"k_rollout_q<1,{q.group(1)},{q.group(2)}>: step loops per role {dict((k, len(v)) for k, v in rl.items())}: NOT ONE PER ROLE"); ok = False
            continue
        for r in range(4):
            c = count(rl[r][0])
            good = c["s_load"] == 0 and c["s_barrier"] == 2
            ok &= good
            print(f"k_rollout_q<1,{q.group(1)},{q.group(2)}> {ROLES[r]}: s_load {c['s_load']} s_barrier {c['s_barrier']}{'' if good else '  FAIL'}")
        c = count(rl[4][0])
        good = c["s_load"] == 0 and c["s_barrier"] == 2 and c["fp64"] == 0 and c["global stores"] > 0
        ok &= good
        print(f"    store loop of <1,{q.group(1)},{q.group(2)}>: scalar loads {c['s_load']}, barriers {c['s_barrier']}, fp64 {c['fp64']}, "
              f"global stores {c['global stores']}{'' if good else '  FAIL'}")
    print("PASS" if ok else "FAIL")
    sys.exit(0 if ok else 1)
if a[:1] == ["--asm"]:
    (pt, pr), (ht, hr) = [(open(a[i]).read(), open(a[i + 1]).read()) for i in (1, 3)]
else:
    pt, pr = listing(a[0])
    ht, hr = listing(a[1] if len(a) > 1 else os.path.join(HERE, ".."))

ok = True
print("python tools/quad_resident_isa.py " + " ".join(x if re.fullmatch(r"[\w./,:=-]+", x) else "'" + x + "'" for x in sys.argv[1:]))
pf, hf = functions(pt), functions(ht)
diff = [n for n in pf if n in hf and pf[n] != hf[n]]
only = sorted(set(pf) ^ set(hf))
print(f"(1) functions: {len(pf)} before, {len(hf)} after; {len(pf) - len(diff) - len([n for n in only if n in pf])} identical instruction for instruction")
for n in diff:
    inside = bool(re.match(r"_ZN3f1611k_rollout_qILi1E", n))
    ok &= inside
    print(f"    differs: {n[:70]}  ({len(pf[n])} -> {len(hf[n])} lines){'' if inside else '  OUTSIDE k_rollout_q<1,*>: FAIL'}")
for n in only:
    ok = False
    print(f"    only {'before' if n in pf else 'after'}: {n[:70]}  FAIL")
print("(2) registers: VGPRs + AGPRs, scratch bytes per lane")
rp, rh = resources(pr), resources(hr)
for k in rh:
    p, h = rp.get(k, {}), rh[k]
    bad = k.startswith("1,") and h["ScratchSize"] > 0
    ok &= not bad
    print(f"    k_rollout_q<{k}>: {p.get('VGPRs')} + {p.get('AGPRs')}, {p.get('ScratchSize')} B  ->  {h['VGPRs']} + {h['AGPRs']}, {h['ScratchSize']} B{'  SCRATCH: FAIL' if bad else ''}")
print("(3) role loops of k_rollout_q<1,*>, before -> after")
for n in hf:
    q = re.match(r"_ZN3f1611k_rollout_qILi1ELb(\d)ELb(\d)E", n)
    if not q or n not in pf: continue
    lp, lh = role_loops(blocks_of_listing(pt, n)), role_loops(blocks_of_listing(ht, n))
    inst = f"1,{q.group(1)},{q.group(2)}"
    for r in range(4):
        tag = f"<1,{q.group(1)},{q.group(2)}> {ROLES[r]}"
        if len(lp.get(r, [])) != 1 or len(lh.get(r, [])) != 1:
            print(f"    {tag}: loops found {len(lp.get(r, []))} -> {len(lh.get(r, []))}  FAIL"); ok = False
            continue
        cp, ch = count(lp[r][0]), count(lh[r][0])
        tp, th = trees(lp[r][0]), trees(lh[r][0])
        only_p, only_h = tp - th, th - tp
        fails, named = [], []
        for role, side, expr in NAMED_TREES:
            if role != r: continue
            c = only_p if side == "before" else only_h
            e = next((e for e in c if (EXPR[e].startswith(expr[:-3]) if expr.endswith("...") else EXPR[e] == expr)), None)
            if e is None: fails.append(f"named tree not among the {side}-only trees: {expr}")
            else:
                c[e] -= 1
                if not c[e]: del c[e]
                named.append(f"{side} only: {expr}")
        same = not only_p and not only_h
        if ch["s_load"]: fails.append("scalar loads in the loop")
        for k in ("lane moves", "v_accvgpr", "64-bit moves", "scratch"):
            if ch[k] > cp[k] + more(inst, r, k): fails.append(f"more {k}")
        if ch["s_barrier"] != 2: fails.append("barriers")
        if not same: fails.append("fp64 trees differ")
        ok &= not fails
        print(f"    {tag}: " + ", ".join(f"{k} {cp[k]} -> {ch[k]}" for k in KEYS)
              + f"; fp64 trees {'identical' if same else f'DIFFER ({sum((only_p + only_h).values())} unmatched)'}"
              + (f" apart from {len(named)} named" if named else "") + (f"  FAIL: {'; '.join(fails)}" if fails else ""))
        for nm in named: print(f"      named, {nm}")
        for side, c in (("before", only_p), ("after", only_h)):
            for e in sorted(c.elements(), key=lambda e: EXPR[e]): print(f"      unmatched, {side} only: {EXPR[e][:400]}")
    st = lh.get(4, [])
    if len(st) != 1:
        print(f"(5) <1,{q.group(1)},{q.group(2)}> store loops found: {len(st)}  FAIL"); ok = False
    else:
        c = count(st[0])
        good = c["s_load"] == 0 and c["s_barrier"] == 2 and c["fp64"] == 0 and c["global stores"] > 0
        ok &= good
        print(f"(5) <1,{q.group(1)},{q.group(2)}> store loop: " + ", ".join(f"{k} {c[k]}" for k in ("instructions", "LDS reads", "s_load", "lane moves", "scratch", "s_barrier", "fp64", "global stores"))
              + ("" if good else "  FAIL"))
    fp, fh = sum(count(lp[r][0])["fp64"] for r in lp if r < 4), sum(count(lh[r][0])["fp64"] for r in lh if r < 4)
    wp, wh = publish_writes(lp[2][0]) if 2 in lp else None, publish_writes(lh[2][0]) if 2 in lh else None
    good = wh is not None and wh <= 3
    ok &= good
    print(f"    <1,{q.group(1)},{q.group(2)}> fp64 instructions per step, four loops: {fp} -> {fh}")
    print(f"(4) <1,{q.group(1)},{q.group(2)}> wave 2: ds_write* between the last fp64 instruction and barrier A: {wp} -> {wh}{'' if good else '  FAIL'}")
print("PASS" if ok else "FAIL")
sys.exit(0 if ok else 1)
