#!/usr/bin/env python3
"""Per-kernel digests of a library's gfx950 code (CPU only, runs nothing on a GPU): whether a source change
moved any kernel's instructions or descriptor.

  python3 tools/isa_digest.py gs_kernels.hip [-o digests.txt]    one line per kernel: sha1  demangled name
  python3 tools/isa_digest.py --compare before.txt after.txt     the kernels that went missing / are new

The .hip file of gpu-solve_amd/csrc is compiled with the command its Makefile rule uses, to device assembly
(--cuda-device-only -S) instead of a shared library. A kernel's text runs from its entry label to the end of
its .amdhsa_kernel descriptor. Comments go, the kernel's own mangled name and the function index of its local
labels (.LBB<i>_<n>, .Lfunc_end<i>) become placeholders, so the digest depends neither on how the template
arguments are spelled nor on the order of instantiation. --compare matches by digest, never by name.
"""
import argparse
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-solve_amd")


def compile_command(src):
    """The Makefile's hipcc command for csrc/<src> (from a dry run), without its link step."""
    dry = subprocess.run(["make", "-C", PKG, "-n", "-B", "ARCH=gfx950", "all"], capture_output=True, text=True,
                         check=True).stdout
    for line in dry.splitlines():
        words = shlex.split(line)
        if words and words[0].endswith("hipcc") and any(w.endswith("csrc/" + src) for w in words):
            out = words.index("-o")
            return [w for i, w in enumerate(words) if w != "-shared" and i not in (out, out + 1)]
    sys.exit(f"no hipcc rule for csrc/{src} in {PKG}/Makefile")


def assembly(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "device.s")
        subprocess.run(compile_command(src) + ["--cuda-device-only", "-S", "-o", out], check=True)
        return open(out).read()


def digests(asm):
    lines = asm.splitlines()
    entry = {line.split(":")[0]: i for i, line in enumerate(lines) if line[:1].isalpha() or line[:1] == "_"}
    rows = []
    for end, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        name = m.group(1)
        start = entry[name]
        while ".end_amdhsa_kernel" not in lines[end]:
            end += 1
        h = hashlib.sha1()
        for text in lines[start:end + 1]:
            text = text.split(";")[0].replace(name, "@KERNEL@")
            text = re.sub(r"\.LBB\d+_", ".LBB@_", re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1@", text))
            text = " ".join(text.split())
            if text:
                h.update(text.encode() + b"\n")
        rows.append((h.hexdigest(), name))
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in rows), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    # the arguments' types say nothing the template arguments do not
    return [(d, re.sub(r"\((Coef|double|int|const|CcPlan).*", "", n.replace("(anonymous namespace)::", "")))
            for (d, _), n in zip(rows, names)]


def read(path):
    return [tuple(line.rstrip("\n").split("  ", 1)) for line in open(path) if line.strip()]


def compare(before, after):
    b, a = read(before), read(after)
    missing = [n for d, n in b if d not in {d for d, _ in a}]
    new = [n for d, n in a if d not in {d for d, _ in b}]
    print(f"{len(b)} kernels before ({len({d for d, _ in b})} distinct), {len(a)} after ({len({d for d, _ in a})} distinct)")
    print(f"missing from after: {len(missing)}")
    for n in missing:
        print("  - " + n)
    print(f"new in after: {len(new)}")
    for n in new:
        print("  + " + n)
    return 1 if new else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src", nargs="?", help="a .hip file of gpu-solve_amd/csrc")
    ap.add_argument("-o", "--output", help="write the digests here instead of printing them")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"), help="two digest files")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not a.src:
        ap.error("a source file or --compare")
    text = "".join(f"{d}  {n}\n" for d, n in digests(assembly(os.path.basename(a.src))))
    if a.output:
        open(a.output, "w").write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
