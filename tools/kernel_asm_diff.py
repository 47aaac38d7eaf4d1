#!/usr/bin/env python3
"""Compare two builds of the library kernel by kernel, from their device assembly: same kernels, same code.

    hipcc -S --cuda-device-only <the Makefile's flags> unit.hip -o dir/unit.s      (tools/asm.sh does this for a list of units)
    python tools/kernel_asm_diff.py <dir A> <dir B>

Every function of every *.s file under the two directories is compared by symbol: kernels, and the few device functions that are not
inlined. What is compared is the instruction stream - labels, instructions, directives inside the function - with comments dropped
and the numbers of local labels replaced by their order of appearance (they count the functions and blocks of the module before
them, so they move when a kernel moves to another unit), and the kernel descriptor (.amdhsa_* block: registers, scratch, LDS).
A plain diff: it looks for no instruction in particular.

Reports the symbols missing from B, extra in B, defined in more than one unit of a side, and those whose code differs (with the first
differing line of each); exit status 1 if there is any."""
import pathlib
import re
import sys
from collections import defaultdict

LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)(\d+)(_\d+)?")


def functions(path):
    """{symbol: (body lines, descriptor lines)} of one assembly file."""
    lines = path.read_text().splitlines()
    types = {m.group(1) for m in (re.match(r"\s*\.type\s+([^,\s]+),@function", l) for l in lines) if m}
    out, desc = {}, {}
    cur = desc_of = None
    for raw in lines:
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", line)
        if m and m.group(1) in types:
            cur = m.group(1)
            out[cur] = []
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = None
            desc_of = m.group(1)
            desc[desc_of] = []
            continue
        if re.match(r"\s*\.end_amdhsa_kernel", line):
            desc_of = None
            continue
        if desc_of is not None:
            desc[desc_of].append(line.strip())
            continue
        if cur is not None:
            if re.match(r"\s*\.size\s+" + re.escape(cur) + r"\b", line) or re.match(r"^\.Lfunc_end\d+:$", line):
                if line.lstrip().startswith(".size"):
                    cur = None
                continue
            if re.match(r"\s*\.(section|text|p2align|globl|weak|protected|hidden|type)\b", line):
                continue
            out[cur].append(line.strip())
    return {s: (normalise(b), desc.get(s, [])) for s, b in out.items()}


def normalise(body):
    """Local label numbers -> order of first appearance inside the function."""
    seen = {}

    def sub(m):
        key = m.group(0)
        if key not in seen:
            seen[key] = f".L{m.group(1)}#{len(seen)}"
        return seen[key]
    return [LOCAL.sub(sub, l) for l in body]


def load(directory):
    where = defaultdict(list)
    code = {}
    files = sorted(pathlib.Path(directory).glob("*.s"))
    if not files:
        sys.exit(f"no *.s files under {directory}")
    for f in files:
        for sym, c in functions(f).items():
            where[sym].append(f.name)
            code.setdefault(sym, c)
    return files, where, code


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    fa, wa, ca = load(sys.argv[1])
    fb, wb, cb = load(sys.argv[2])
    kern = lambda code: sum(1 for c in code.values() if c[1])                   # noqa: E731  (functions with a kernel descriptor)
    print(f"A: {len(fa)} unit(s), {len(ca)} functions, {kern(ca)} kernels")
    print(f"B: {len(fb)} unit(s), {len(cb)} functions, {kern(cb)} kernels")
    for f in fb:
        print(f"   {f.name}: {sum(1 for s, w in wb.items() if f.name in w and cb[s][1])} kernels")
    missing = sorted(set(ca) - set(cb))
    extra = sorted(set(cb) - set(ca))
    dup = sorted((s, w) for side in (wa, wb) for s, w in side.items() if len(w) > 1)
    differ = []
    for s in sorted(set(ca) & set(cb)):
        if ca[s] != cb[s]:
            a, b = ca[s][0] + ca[s][1], cb[s][0] + cb[s][1]
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            differ.append((s, first, a[first] if first < len(a) else "<end>", b[first] if first < len(b) else "<end>"))
    print(f"missing from B: {len(missing)}")
    for s in missing:
        print("   ", s)
    print(f"extra in B: {len(extra)}")
    for s in extra:
        print("   ", s)
    print(f"defined in more than one unit: {len(dup)}")
    for s, w in dup:
        print("   ", s, w)
    print(f"code differs: {len(differ)}")
    for s, i, x, y in differ:
        print(f"    {s}\n      line {i}: A: {x}\n      {' ' * len(str(i))}       B: {y}")
    same = len(set(ca) & set(cb)) - len(differ)
    print(f"identical: {same} of {len(ca)} functions")
    sys.exit(1 if missing or extra or dup or differ else 0)


if __name__ == "__main__":
    main()
