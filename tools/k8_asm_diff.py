"""Compare the K7 / K8 kernels of two gfx950 assembly listings of csrc/k7_export.hip (hipcc ... --cuda-device-only -S):
    python tools/k8_asm_diff.py before.s after.s
Instruction streams are compared from each kernel's label to its end, with comments, directives and local label numbers stripped.  Prints,
per kernel, whether `after` equals `before`, and both listings' resources: VGPRs, SGPRs, bytes of scratch, bytes of LDS.  The scanline kernels
are matched across the two spellings k8_png_rows / k8_png_rows_m (two kernels) and k8_png_rows<false> / <true> (one template)."""
import re
import subprocess
import sys


def short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\((K\w+Args)\)$", "", name)
    name = re.sub(r"^(k8_\w+_rows)_m$", r"\1<true>", name)
    return re.sub(r"^(k8_\w+_rows)$", r"\1<false>", name)


def listing(path):
    """{kernel: ([instruction lines], (vgprs, sgprs, scratch, lds))}"""
    text = open(path).read()
    res = {}
    for block in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:  # one block of the metadata per kernel
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        res[name] = (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"), get("group_segment_fixed_size"))
    out = {}
    for mangled, r in res.items():
        m = re.search(r"^%s:[^\n]*\n(.*?)\n\.Lfunc_end\d+:" % re.escape(mangled), text, re.S | re.M)
        lines = []
        for line in m.group(1).split("\n"):
            line = line.split(";")[0].rstrip()
            if not line.strip() or line.strip().startswith("."):
                continue
            lines.append(re.sub(r"\.?LBB\d+_", "LBB_", line))
        out[short(mangled)] = (lines, r)
    return out


if __name__ == "__main__":
    before, after = listing(sys.argv[1]), listing(sys.argv[2])
    for name in sorted(set(before) | set(after)):
        b, a = before.get(name), after.get(name)
        if not a or not b:
            print("%-40s only in %s" % (name, "before" if b else "after"))
            continue
        fmt = lambda r: "%3d VGPRs %3d SGPRs %d B scratch %5d B LDS" % r  # noqa: E731
        print("%-40s %-9s %5d -> %5d instructions | %s -> %s" % (name, "identical" if a[0] == b[0] else "DIFFERENT", len(b[0]), len(a[0]), fmt(b[1]), fmt(a[1])))
