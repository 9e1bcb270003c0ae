"""Compare the k0_aov_pack instantiations of two gfx950 assembly listings of csrc/k0_import.hip (hipcc ... --cuda-device-only -S):
    python tools/k0_aov_asm_diff.py before.s after.s
Instruction streams are compared with symbol names and local label numbers normalised; prints, per SET, whether the default instantiation of
`after` equals the one of `before`, and the resources (VGPRs, SGPRs, scratch bytes) of every instantiation of `after`."""
import re
import sys


def kernels(path):
    """{(SET, conventions in use): [instruction lines]}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN[^\n:]*k0_aov_packILi(\d)E(?:Lb(\d)E)?[^\n:]*):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        _, set_, conv, body = m.groups()
        lines = []
        for line in body.split("\n"):
            line = line.split(";")[0].rstrip()
            if not line.strip() or line.strip().startswith("."):
                continue
            line = re.sub(r"_ZN\w*k0_aov_pack\w*", "K", line)
            lines.append(re.sub(r"\.?LBB\d+_", "LBB_", line))
        out[(int(set_), int(conv or 0))] = lines
    return out


def resources(path):
    text = open(path).read()
    res = {}
    for m in re.finditer(r"\.name:\s+(_ZN\S*k0_aov_packILi(\d)E(?:Lb(\d)E)?\S*)(.*?)\.wavefront_size", text, re.S):
        block = m.group(4)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
        res[(int(m.group(2)), int(m.group(3) or 0))] = (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"))
    return res


if __name__ == "__main__":
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    for s in (0, 1, 2):
        a, b = before[(s, 0)], after[(s, 0)]
        print("SET %d default: %d -> %d instructions, %s" % (s, len(a), len(b), "identical" if a == b else "DIFFERENT"))
    for key, (v, sg, scratch) in sorted(resources(sys.argv[2]).items()):
        print("SET %d conventions %d: %d instructions, %d VGPRs, %d SGPRs, %d bytes of scratch" % (key + (len(after[key]), v, sg, scratch)))
