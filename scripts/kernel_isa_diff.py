#!/usr/bin/env python3
"""Compare the kernels of two device assembly files, whatever their names.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S a.hip -o a.s
    scripts/kernel_isa_diff.py a.s b.s            # exit status 0: every kernel of either file has a partner in the other

A kernel is its instruction stream with comments, assembler directives and blank lines dropped, local labels renumbered in
order of appearance and symbol names replaced, plus the resource fields of its metadata entry (registers, spills, scratch,
LDS, workgroup size).  Kernels are paired by the hash of that text: a refactoring that only renames or re-parameterises a
kernel leaves every hash where it was.  Kernels left without a partner are listed with the first line at which they differ
from the closest unpaired kernel of the other file.  (Several .s files of one build: concatenate them.)

Names are printed demangled where c++filt is present and knows the mangling, and mangled otherwise (binutils' c++filt does not know
the _Float16 / __bf16 template arguments: a mix of both forms in one listing is expected).

The tool compares text only; it knows nothing about the instruction set.
"""
import hashlib
import re
import shutil
import subprocess
import sys

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size", ".max_flat_workgroup_size")
LABEL = re.compile(r"\.L[A-Za-z0-9_$.]+")


def parse(path):
    """{kernel name: (normalised lines, {field: value})} of one .s file"""
    lines = open(path, errors="replace").read().split("\n")
    meta, cur = {}, None                                     # metadata entries: "  - .key: v" opens one, "    .key: v" continues it
    for ln in lines:
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip()
        if m.group(2) == ".name":
            meta[cur[".name"]] = cur
    kernels = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", lines[i])
        if not m or m.group(1) not in meta:
            i += 1
            continue
        name, body, labels = m.group(1), [], {}
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            s = lines[i].split(";", 1)[0].strip()
            i += 1
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue                                     # blank, comment or directive
            s = LABEL.sub(lambda l: labels.setdefault(l.group(0), "L%d" % len(labels)), s)
            body.append(re.sub(r"\s+", " ", s.replace(name, "SELF")))
        known = set(meta)
        body = [" ".join("SYM" if w.rstrip(",") in known else w for w in b.split(" ")) for b in body]
        kernels[name] = (body, {f: meta[name].get(f, "-") for f in FIELDS})
    return kernels


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: (o.replace("use::", "").replace("(use::ConvArgs)", "").replace("void ", "") if o else n) for n, o in zip(names, out)}


def key(k):
    body, fields = k
    return hashlib.sha256(("\n".join(body) + "\n" + repr(sorted(fields.items()))).encode()).hexdigest()


def first_difference(a, b):
    (ba, fa), (bb, fb) = a, b
    for n, (x, y) in enumerate(zip(ba, bb)):
        if x != y:
            return n, "instruction %d: '%s' | '%s'" % (n, x, y)
    if len(ba) != len(bb):
        n = min(len(ba), len(bb))
        return n, "instruction %d: one stream ends (%d | %d instructions)" % (n, len(ba), len(bb))
    d = ["%s %s | %s" % (f, fa[f], fb[f]) for f in FIELDS if fa[f] != fb[f]]
    return len(ba), "same instructions; " + ", ".join(d)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    A, B = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(list(A) + list(B))
    by_key = {}
    for n, k in B.items():
        by_key.setdefault(key(k), []).append(n)
    pairs, left_a = [], []
    for n, k in A.items():
        c = by_key.get(key(k))
        if c:
            pairs.append((n, c.pop(0)))
        else:
            left_a.append(n)
    left_b = [n for c in by_key.values() for n in c]
    print("%s: %d kernels, %s: %d kernels, paired: %d" % (sys.argv[1], len(A), sys.argv[2], len(B), len(pairs)))
    for a, b in pairs:
        body, f = A[a]
        print("  = %s\n    %s\n    %d instructions, sha256 %s, %s" % (names[a], names[b], len(body), key(A[a])[:16],
                                                                     " ".join("%s=%s" % (x[1:], f[x]) for x in FIELDS)))
    for side, left, own, other, rest in (("<", left_a, A, B, left_b), (">", left_b, B, A, left_a)):
        for n in left:
            print("  %s %s: no partner" % (side, names[n]))
            if rest:
                pos, text, m = max((first_difference(own[n], other[o]) + (o,) for o in rest), key=lambda t: t[0])
                print("    closest %s\n    %s" % (names[m], text))
    return 1 if left_a or left_b else 0


if __name__ == "__main__":
    sys.exit(main())
