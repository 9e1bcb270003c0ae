#!/usr/bin/env python3
"""Development helper (build container): are the kernels of two builds the same machine code?  For a change that moves kernels between files.

    python tools/compare_kernels.py old_dir new_dir

Each directory holds the gfx950 assembly of every translation unit (`hipcc $(HIPFLAGS) -S --cuda-device-only x.hip -o dir/x.s`, each file with its own
contraction flag from csrc/sources.mk).  Functions, data objects and code-object metadata entries are keyed by their (mangled) name, not by file, and
compared as text: a kernel's instructions with the resource lines behind them, its kernel descriptor, its metadata entry.  What only records the position
in a file is normalised first: the function's index in local labels (.LBB<n>_<m>, .LJTI<n>_<m>, .Lfunc_end<n>), the file-wide .Ltmp counter, the
per-file __hip_cuid_* symbol; .file / .ident lines lie outside every compared piece.  Prints the names that differ or exist on one side only, then the
counts; exit status 1 if anything differs.
"""
import glob
import os
import re
import sys


def normalise(text):
    text = re.sub(r"[ \t]+", " ", text)  # (the column a comment starts in follows the width of the label before it)
    text = re.sub(r"(?<![\w.])(\.?)(LBB|BB|LJTI|LCPI)\d+_", r"\1\2_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)
    seen = {}
    return re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % seen.setdefault(m.group(0), len(seen)), text)


def pieces(directory):
    """{(kind, name): normalised text}; kinds: code, descriptor, metadata, object.  kernels: the names that have a descriptor."""
    out, kernels = {}, set()
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text = open(path).read()
        # file-local objects of one name (`.table`, `.table.30`): the suffix counts the file's unnamed values, so number them in order instead
        count = {}
        for base, n in re.findall(r"^(\.[A-Za-z_]\w*)\.(\d+):", text, re.M):
            count[base] = count.get(base, 0) + 1
            text = re.sub(r"%s\.%s\b" % (re.escape(base), n), "%s.dup%d" % (base, count[base]), text)
        for m in re.finditer(r"; -- Begin function (\S+)\n(.*?); -- End function", text, re.S):
            name, body = m.group(1), m.group(2)
            d = re.search(r"\t\.amdhsa_kernel .*?\.end_amdhsa_kernel\n", body, re.S)
            if d:
                kernels.add(name)
                out[("descriptor", name)] = normalise(d.group(0))
                body = body[:d.start()] + body[d.end():]
            out[("code", name)] = normalise(body)
        for m in re.finditer(r"\t\.type\t(\S+),@object.*?\n\t\.size\t\1, \d+\n", text, re.S):
            if not m.group(1).startswith("__hip_cuid"):
                out[("object", m.group(1))] = normalise(m.group(0))
        meta = text[text.rfind("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
        meta = meta.split("\namdhsa.target:")[0]
        for block in re.split(r"\n  - ", meta)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            out[("metadata", name)] = normalise(block)
    return out, kernels


def main(old_dir, new_dir):
    (old, old_k), (new, new_k) = pieces(old_dir), pieces(new_dir)
    bad = set()
    for key in sorted(set(old) | set(new)):
        if key not in old or key not in new:
            print("%-10s %s: only in %s" % (key[0], key[1], new_dir if key in new else old_dir))
        elif old[key] != new[key]:
            print("%-10s %s: differs" % key)
        else:
            continue
        bad.add(key[1])
    others = {name for kind, name in set(old) | set(new) if name not in old_k | new_k}
    print("%d kernels (%d old, %d new), %d differ; %d other functions and objects, %d differ" %
          (len(old_k | new_k), len(old_k), len(new_k), len(bad & (old_k | new_k)), len(others), len(bad & others)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
