#!/usr/bin/env python3
"""The vmcnt waits of a kernel's loops, read from device assembly (CPU only, runs nothing on a GPU): per loop, every
`s_waitcnt vmcnt(N)` in layout order from the loop's header on, with the instruction that follows it, the number of
register copies (v_mov_b32 / v_mov_b64) that follow it without a break, and whether it sits in a back-edge block.

  python3 tools/waits_table.py device.s 'k_tb3y<true, true, true, true>'

device.s: gs_kernels.hip compiled with the Makefile's flags plus `--cuda-device-only -S` (tools/isa_digest.py has the
command). The kernel is named as c++filt prints it, without its arguments; a unique substring is enough. A block belongs
to the loop its label's comment names (`in Loop: Header=BBi_n Depth=1`, or `Parent Loop BBi_n Depth=1` for a nested one);
a back-edge block is one that branches to the header's label or falls through into it. Only waits and copies are read:
what a wait waits FOR is for the reader to work out from the loads and stores around it.
"""
import re
import subprocess
import sys

WAIT = re.compile(r"s_waitcnt\b.*\bvmcnt\((\d+)\)")
COPY = re.compile(r"v_mov_b(32|64)(_e32|_e64)?\s")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BLOCK = re.compile(r"^; %bb\.\d+:")
BRANCH = re.compile(r"\s(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")


def kernel_text(lines, want):
    """(demangled name, the lines from the kernel's entry label to its .Lfunc_end)."""
    kernels = {line.split()[-1] for line in lines if ".amdhsa_kernel" in line}
    entries = [(i, m.group(1)) for i, line in enumerate(lines)
               if (m := re.match(r"^(_Z\w+):", line)) and m.group(1) in kernels]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in entries), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    hits = [(i, n) for (i, _), n in zip(entries, names) if want in n.replace("(anonymous namespace)::", "")]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels match {want!r}: " +
                 ", ".join(n.replace("(anonymous namespace)::", "").split("(")[0] for _, n in hits))
    start, name = hits[0]
    end = start
    while not lines[end].startswith(".Lfunc_end"):
        end += 1
    return re.sub(r"\((Coef|double|int|const).*", "", name.replace("(anonymous namespace)::", "")), lines[start:end]


def blocks(text):
    """[label or None, loop header or None, [instruction, ...]] per basic block, in layout order."""
    out = [[None, None, []]]
    for line in text[1:]:
        m = LABEL.match(line)
        if m or BLOCK.match(line):
            loop = re.search(r"(?:Parent Loop|Header=)\s*(BB\d+_\d+) Depth=1", line)
            if loop:
                head = "." + "L" + loop.group(1)
            elif m and "Loop Header: Depth=1" in line:
                head = m.group(1)
            else:
                head = None
            out.append([m.group(1) if m else None, head, []])
            continue
        if line.startswith(";") and "Parent Loop" in line and out[-1][1] is None:
            loop = re.search(r"Parent Loop (BB\d+_\d+) Depth=1", line)
            if loop:
                out[-1][1] = ".L" + loop.group(1)
            continue
        ins = line.split(";")[0].strip()
        if ins and not ins.startswith("."):
            out[-1][2].append(ins)
    return out


def table(name, bl):
    print(name)
    heads = []
    for _, head, _ in bl:
        if head and head not in heads:
            heads.append(head)
    if not heads:
        print("  no loops")
    for n, head in enumerate(heads):
        idx = [i for i, b in enumerate(bl) if b[1] == head]
        hi = next(i for i in idx if bl[i][0] == head)
        order = [i for i in idx if i >= hi] + [i for i in idx if i < hi]
        latch = set()
        for i in idx:
            ins = bl[i][2]
            if any((m := BRANCH.search(" " + s)) and m.group(2) == head for s in ins):
                latch.add(i)
            if i + 1 == hi and not (ins and ins[-1].startswith("s_branch")):
                latch.add(i)
        rows = []
        for i in order:
            ins = bl[i][2]
            for j, s in enumerate(ins):
                m = WAIT.search(s)
                if not m:
                    continue
                after = ins[j + 1] if j + 1 < len(ins) else "(end of block)"
                copies = 0
                while j + 1 + copies < len(ins) and COPY.match(ins[j + 1 + copies] + " "):
                    copies += 1
                rows.append((int(m.group(1)), i in latch, copies, " ".join(after.split())))
        ncopy = sum(1 for i in latch for s in bl[i][2] if COPY.match(s + " "))
        nwait = sum(1 for r in rows if r[1])
        print(f"  loop {n + 1} (header {head}, {len(idx)} blocks): vmcnt " + " ".join(str(r[0]) for r in rows))
        print(f"    lowest vmcnt {min((r[0] for r in rows), default='-')}; back-edge blocks: {ncopy} copies, "
              f"{nwait} vmcnt waits")
        for v, back, copies, after in rows:
            print(f"    vmcnt({v}){' [back-edge]' if back else ''}  ->  {after}" + (f"  (+{copies} copies)" if copies else ""))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    lines = open(sys.argv[1]).read().splitlines()
    name, text = kernel_text(lines, sys.argv[2])
    table(name, blocks(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
