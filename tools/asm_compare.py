"""Per-kernel comparison of two `make asm` outputs (profiles/*/asm_compare.txt): function bodies with label
numbers normalised, and the kernel-resource-usage blocks.  A parent kernel is paired with the new kernel of
the same name, or of the same name with template arguments `, false` appended.
usage: python tools/asm_compare.py PARENT_CSRC_DIR NEW_CSRC_DIR [KERNEL: print that body's diff]"""
import re
import shutil
import subprocess
import sys


def demangle(names):
    out = subprocess.run([shutil.which("c++filt") or "llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True).stdout
    return dict(zip(names, out.splitlines()))


def short(d):
    d = d.replace("(anonymous namespace)::", "")
    d = re.sub(r"^void ", "", d)
    depth = 0
    for i, ch in enumerate(d):       # cut at the argument list's '(' (outside template brackets)
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return d[:i]
    return d


def bodies(path):
    fn, cur, res = None, [], {}
    for ln in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if fn is None:
            if m and not m.group(1).startswith(".L") and m.group(1).startswith("_Z"):
                fn, cur = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            res[fn] = cur
            fn = None
            continue
        s = ln.split(";")[0].rstrip()
        if not s.strip():
            continue
        s = re.sub(r"\.(LBB|Ltmp|Lfunc_end|Lfunc_begin)\d+(_\d+)?", r".\1N", s)
        cur.append(s.replace(fn, "SELF"))
    return res


def resources(path):
    res, fn = {}, None
    for ln in open(path):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
            res[fn] = []
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w \[\]/]*): (\S+)", ln)
        if m and fn:
            res[fn].append((m.group(1).strip(), m.group(2)))
    return res


def load(d):
    b = bodies(d + "/pii_engine.s")
    r = resources(d + "/resource_usage.txt")
    dm = demangle(sorted(set(b) | set(r)))
    return ({short(dm[k]): v for k, v in b.items() if k in r}, {short(dm[k]): v for k, v in r.items()})


pb, pr = load(sys.argv[1])
nb, nr = load(sys.argv[2])


def twin(n):          # a parent kernel's name in the new build: new template parameters default to false
    for cand in (n, n[:-1] + ", false>" if n.endswith(">") else None, n[:-1] + ", false, false>" if n.endswith(">") else None):
        if cand and cand in nb:
            return cand
    return None


pairs = {n: twin(n) for n in pb}
matched_new = {v for v in pairs.values() if v}
print(f"kernels: parent {len(pb)}, new {len(nb)}")
print("only in parent:", [n for n, v in pairs.items() if not v])
print("only in new:", [n for n in nb if n not in matched_new])
nd = nrd = tot = 0
diffs = []
for n, v in pairs.items():
    if not v:
        continue
    tot += len(pb[n])
    bd, rd = pb[n] != nb[v], pr[n] != nr[v]
    nd += bd
    nrd += rd
    if bd or rd:
        diffs.append((n, v, bd, rd))
print(f"kernels in both: {len(matched_new)}; function bodies differing: {nd}; resource blocks differing: {nrd}")
print(f"instructions and directives compared: {tot}")
print("\nrenamed for the comparison (parent -> new):")
for n, v in pairs.items():
    if v and v != n:
        print(f"  {n} -> {v}")
print("\nkernels in both whose body or resource block differs:")
for n, v, bd, rd in diffs:
    print(f"  {n} -> {v}: body {'differs' if bd else 'same'} ({len(pb[n])} -> {len(nb[v])} lines)")
    for (k, a), (_, b) in zip(pr[n], nr[v]):
        print(f"      {k}: {a} -> {b}")
print("\nkernels only in new (resource block):")
for n in nb:
    if n not in matched_new:
        print(f"  {n}: body {len(nb[n])} lines")
        for k, a in nr[n]:
            print(f"      {k}: {a}")

if len(sys.argv) > 3:
    import difflib
    n = sys.argv[3]
    for ln in difflib.unified_diff(pb[n], nb[pairs[n]], lineterm="", n=1):
        print(ln)
