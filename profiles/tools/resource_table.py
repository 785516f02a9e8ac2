"""Resource table of the SENT lane-per-graph kernels from two compiler logs (parent commit, this commit).

Each log is the output of
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -c -Iinclude -Rpass-analysis=kernel-resource-usage \
        glearning-benchmark_amd/csrc/gtok_sent.hip
Usage: python profiles/tools/resource_table.py PARENT.log BRANCH.log > profiles/blane_pack/sent_kernel_resources.md
"""
import re
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "SGPRs Spill", "VGPRs Spill"]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def targs(name):
    """template arguments of a mangled kernel name: Li4E -> 4, Lb1E -> 1; a missing trailing default (PACK, PK8, TOK8) -> 0"""
    return [x[2:-1] for x in re.findall(r"L[ib]\d+E", name)]


def main():
    parent, branch = parse(sys.argv[1]), parse(sys.argv[2])
    for kern, cols, n in (("sent_blane_kernel", "W P U16 PACK", 4), ("sent_lane_kernel", "LAB P REMAP PK U16 PACK PK8 TOK8", 8)):
        print(f"## `{kern}`\n")
        print(f"| {cols} | VGPRs | AGPRs | SGPRs (total) | scratch bytes / lane | waves / SIMD | static LDS | SGPR spills | VGPR spills | against the parent |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for name, r in branch.items():
            if kern not in name:
                continue
            a = targs(name)
            a += ["0"] * (n - len(a))
            # the parent's name of the same instantiation: a trailing `false` default was not spelled there
            old = parent.get(name) or parent.get(re.sub(r"Lb0E(E+vNS_\d+Sent\w+ArgsE)$", r"\1", name))
            verdict = "new" if old is None else ("identical" if all(old.get(f) == r.get(f) for f in FIELDS) else
                                                 "CHANGED: " + ", ".join(f"{f} {old.get(f)} -> {r.get(f)}" for f in FIELDS if old.get(f) != r.get(f)))
            print("| " + " ".join(a) + " | " + " | ".join(r.get(f, "?") for f in FIELDS) + f" | {verdict} |")
        print()


if __name__ == "__main__":
    main()
