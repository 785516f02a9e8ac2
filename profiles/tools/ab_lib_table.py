"""Tables of profiles/tools/ab_lib.sh's output: per figure, every process's value, the median and the range of each side, and whether the
branch's median lies inside the parent's own min-max range or on the better side of it.  python profiles/tools/ab_lib_table.py OUT_DIR"""
import glob, json, statistics, sys
out = sys.argv[1]
FIG = {
 "full": [("ibtt.kernel_ms", ("ibtt", "kernel_ms"), 1), ("ibtt graphs/s (wall)", ("ibtt", "graphs_per_sec_per_gpu"), 0),
          ("boundary.ibtt_tokenize_csr resident graphs/s", ("boundary", "ibtt_tokenize_csr", "resident_graphs_per_sec"), 0),
          ("boundary.ibtt_token_dataset_init s", ("boundary", "ibtt_token_dataset_init", "seconds"), 1),
          ("boundary.ibtt_vocab_scan s", ("boundary", "ibtt_vocab_scan", "seconds"), 1),
          ("boundary.ibtt_strings s", ("boundary", "ibtt_strings", "seconds"), 1),
          ("boundary.ibtt_dataloader items/s", ("boundary", "ibtt_dataloader", "items_per_sec"), 0),
          ("ms_per_step (SENT headline)", ("ms_per_step",), 1)],
 "er": [("ibtt.kernel_ms (ibtt_synth)", ("ibtt", "kernel_ms"), 1), ("ibtt graphs/s", ("ibtt", "graphs_per_sec_per_gpu"), 0),
        ("text_to_ids.kernel_ms", ("text_to_ids", "kernel_ms"), 1), ("text_to_ids graphs/s", ("text_to_ids", "graphs_per_sec_per_gpu"), 0),
        ("vocab_stats.kernel_ms", ("vocab_stats", "kernel_ms"), 1), ("vocab_stats graphs/s", ("vocab_stats", "graphs_per_sec_per_gpu"), 0),
        ("ms_per_step (SENT headline)", ("ms_per_step",), 1)],
}
def vals(leg, side, path):
    v = []
    for f in sorted(glob.glob(f"{out}/{leg}_{side}_*.json")):
        try:
            d = json.loads(open(f).read())
            for k in path: d = d[k]
            v.append(float(d))
        except Exception as e:
            v.append(float("nan"))
    return v
fmt = lambda v: ", ".join(f"{x:.5g}" for x in v)
print("| leg | figure | lower is better | parent: values, median [min .. max] | branch: values, median | branch median within the parent's range or better |")
print("|---|---|---|---|---|---|")
for leg, figs in FIG.items():
    for name, path, sense in figs:
        a, b = vals(leg, "parent", path), vals(leg, "branch", path)
        if not a or not b: continue
        lower = sense != 0
        ma, mb = statistics.median(a), statistics.median(b)
        ok = mb <= max(a) if lower else mb >= min(a)
        print(f"| {leg} | {name} | {'yes' if lower else 'no'} | {fmt(a)}: {ma:.5g} [{min(a):.5g} .. {max(a):.5g}] | {fmt(b)}: {mb:.5g} | {'yes' if ok else 'NO'} |")
# host
keys = None
rows = {}
for side in ("parent", "branch"):
    for f in sorted(glob.glob(f"{out}/host_{side}_*.json")):
        d = json.loads(open(f).read())["us_per_call"]
        for k, v in d.items(): rows.setdefault(k, {}).setdefault(side, []).append(v)
print("\n| entry point (us per call) | parent: values, median [min .. max] | branch: values, median | branch median within the parent's range or below |")
print("|---|---|---|---|")
for k, r in rows.items():
    a, b = r.get("parent", []), r.get("branch", [])
    if a and b:
        print(f"| {k} | {fmt(a)}: {statistics.median(a):.5g} [{min(a):.5g} .. {max(a):.5g}] | {fmt(b)}: {statistics.median(b):.5g} | {'yes' if statistics.median(b) <= max(a) else 'NO'} |")
