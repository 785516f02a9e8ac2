"""Table of profiles/tools/ab_trees.sh's output: per figure, every process's value, the median and the range of each tree, and whether
the branch's median lies inside the parent's own min-max range (or below it).  python profiles/tools/ab_trees_table.py OUT_DIR"""
import glob
import json
import statistics
import sys

FIGURES = [("headline", "ms_per_step", ("ms_per_step",)),
           ("full", "ms_per_step", ("ms_per_step",)),
           ("full", "boundary.torch_op_sent.ms_per_step", ("boundary", "torch_op_sent", "ms_per_step")),
           ("full", "epoch_loop.ms_per_epoch", ("epoch_loop", "ms_per_epoch")),
           ("subset", "zinc_subset ms_per_step", ("ms_per_step",))]


def values(out, leg, tree, path):
    vals = []
    for f in sorted(glob.glob(f"{out}/{leg}_{tree}_*.json")):
        d = json.loads(open(f).read())
        for k in path:
            d = d[k]
        vals.append(float(d))
    return vals


def main(out):
    print("| leg | figure (ms) | parent: values, median [min .. max] | branch: values, median | branch median inside the parent's range or below |")
    print("|---|---|---|---|---|")
    for leg, name, path in FIGURES:
        a, b = values(out, leg, "parent", path), values(out, leg, "branch", path)
        if not a or not b:          # a leg the run left out
            continue
        ma, mb = statistics.median(a), statistics.median(b)
        fmt = lambda v: ", ".join(f"{x:.5f}" for x in v)
        print(f"| {leg} | {name} | {fmt(a)}: {ma:.5f} [{min(a):.5f} .. {max(a):.5f}] | {fmt(b)}: {mb:.5f} | {'yes' if mb <= max(a) else 'NO'} |")


if __name__ == "__main__":
    main(sys.argv[1])
