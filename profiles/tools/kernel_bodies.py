"""Compare the kernels of two builds - the parent commit's and this commit's - file by file moved or not: the compiler's resource
report of every kernel and the kernel's body in the device assembly.

Each directory holds what these commands leave, one per source file (run inside the directory):
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage --save-temps -c -I<repo>/include \
        -o gtok_ibtt.o <repo>/glearning-benchmark_amd/csrc/gtok_ibtt.hip > gtok_ibtt.log 2>&1
i.e. NAME.log (the remarks) and NAME-hip-amdgcn-amd-amdhsa-gfx950.s.  Kernels are matched by mangled name across all files of a
directory, so a kernel that moved to another source file is compared with itself.  A body runs from the kernel's label to its
.Lfunc_end; comments are dropped and .LBB<n>_ becomes .LBB_ (the function index moves with the file).

Usage: python profiles/tools/kernel_bodies.py PARENT_DIR BRANCH_DIR > profiles/ibtt_split/kernel_resources.md
Exit status 1 when a kernel of the parent is missing, or differs in a resource or in its body.
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill"]

HEADER = """# Kernels of two builds compared: resources and bodies

Both trees compiled file by file with the remarks and the temporaries kept (run inside an empty directory per tree; `<tree>` is a
checkout of the parent commit, then of this one; a file one tree lacks is left out there):

    for f in gtok_ibtt gtok_text gtok_rows gtok_sent; do
      hipcc -O3 -std=c++17 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage --save-temps -c -I<tree>/include \\
          -o $f.o <tree>/glearning-benchmark_amd/csrc/$f.hip > $f.log 2>&1
    done
    python profiles/tools/kernel_bodies.py PARENT_DIR BRANCH_DIR > profiles/ibtt_split/kernel_resources.md

Kernels are matched by mangled name, so one that moved to another file is compared with itself: the compiler's resource report,
and the body in the device assembly from the kernel's label to its `.Lfunc_end` with comments dropped and `.LBB<n>_` written
`.LBB_` (the function index moves with the file).
"""


def resources(directory):
    """{mangled kernel name: (source file, {field: value})} from the remarks of every NAME.log"""
    out, cur = {}, None
    for path in sorted(glob.glob(os.path.join(directory, "*.log"))):
        for line in open(path):
            m = re.search(r"remark:\s+\S*?([\w.]+\.hip):\d+:\d+:\s+Function Name: (\S+)", line)
            if m:
                cur = m.group(2)
                out[cur] = (m.group(1), {})
                continue
            m = re.search(r"remark:.*?:\d+:\d+:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
            if m and cur:
                out[cur][1][m.group(1).strip()] = m.group(2)
    return out


def bodies(directory):
    """{mangled kernel name: [normalised assembly lines]} from every device .s"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        name, body = None, None
        for line in open(path):
            line = line.split(";", 1)[0].rstrip()
            m = re.match(r"^(\w+):$", line)
            if name is None and m:
                name, body = m.group(1), []
                continue
            if name is not None:
                if re.match(r"^\.Lfunc_end\d+:$", line):
                    out[name] = body
                    name = None
                elif line:
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def demangle(names):
    try:
        text = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        # (a kernel of an unnamed namespace demangles to "(anonymous namespace)::name<..>(..)": that prefix goes before the cut at the argument list)
        return dict(zip(names, (re.sub(r"^void |\(.*$", "", t.replace("(anonymous namespace)::", "")).replace("gtok::", "") for t in text)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    pres, bres, pbody, bbody = resources(sys.argv[1]), resources(sys.argv[2]), bodies(sys.argv[1]), bodies(sys.argv[2])
    pretty = demangle(sorted(set(pres) | set(bres)))
    print(HEADER)
    print("| kernel | parent file | file | VGPRs | AGPRs | SGPRs | scratch | LDS | waves / SIMD | SGPR spills | VGPR spills | resources | body (lines) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    bad = 0
    for name, (pfile, old) in pres.items():
        if name not in bres:
            print(f"| `{pretty[name]}` | {pfile} | MISSING |" + " |" * 10)
            bad += 1
            continue
        bfile, new = bres[name]
        same_res = all(old.get(f) == new.get(f) for f in FIELDS)
        res = "identical" if same_res else "CHANGED: " + ", ".join(f"{f} {old.get(f)} -> {new.get(f)}" for f in FIELDS if old.get(f) != new.get(f))
        same_body = name in pbody and pbody[name] == bbody.get(name)
        body = f"identical ({len(pbody[name])})" if same_body else "DIFFERENT"
        bad += (not same_res) + (not same_body)
        print(f"| `{pretty[name]}` | {pfile} | {bfile} | " + " | ".join(new.get(f, "?") for f in FIELDS) + f" | {res} | {body} |")
    extra = [n for n in bres if n not in pres]
    moved = {}
    for name, (pfile, _) in pres.items():
        if name in bres and bres[name][0] != pfile:
            moved[(pfile, bres[name][0])] = moved.get((pfile, bres[name][0]), 0) + 1
    print(f"\n{len(pres)} kernels in the parent's files, {len(bres)} in this commit's; {len(extra)} only here; {bad} differences.  Moved: "
          + ("; ".join(f"{n} from {a} to {b}" for (a, b), n in sorted(moved.items())) or "none") + ".")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
