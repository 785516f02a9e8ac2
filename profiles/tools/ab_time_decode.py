"""The decoders' kernels timed on two builds of the library side by side: the parent's (profiles/tools/ab_build.sh <ref> parent) and
the tree's own.  Gated: exit status 1 when a phase of the tree's build is slower than the parent's by more than the parent's spread.

    python profiles/tools/ab_time_decode.py PARENT_LIB OUT_DIR [JOB ...]     (then copy OUT_DIR/timing.md to profiles/<name>/)
    python profiles/tools/ab_time_decode.py --report OUT_DIR                  (timing.md again, from the ab_*.json of earlier runs)

JOB: sent:zinc sent:config5 (the phases of time_sent_decode_csr.py's new route), ibtt:zinc ibtt:config5 (sizes / csr of
time_ibtt_decode.py), twice (the twice-parsed SENT path, which those two do not reach: 4,000 labelled molecules decoded with
max_num_nodes = 16,384 - the row cursors fill the workgroup's LDS, nothing is staged, every row is parsed a second time).  Default:
all five.  A job starts PROCS fresh processes per side, each under a time limit of its own, the parent's library (GTOK_LIB) first
in even rounds and the tree's first in odd ones; a process reports the median of each phase.  Per phase: the tree's median of
the processes' medians may exceed the parent's by no more than the parent's own spread (largest - smallest of its processes'
medians).  A process that fails stops the run."""
import importlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PROCS, REPEATS = int(os.environ.get("PROCS", 3)), int(os.environ.get("REPEATS", 7))
LIMIT = int(os.environ.get("CHILD_LIMIT", 240))       # seconds per process
JOBS = ("sent:zinc", "sent:config5", "ibtt:zinc", "ibtt:config5", "twice")
med = lambda v: sorted(v)[len(v) // 2]


def twice_child() -> dict:
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import time_sent_decode_csr as tsd
    gtok = importlib.import_module("glearning-benchmark_amd")
    dev, maxn = torch.device("cuda:0"), gtok._lib.SENT_LARGE_MAX_NODES
    d = gtok.synth.zinc_like(4000, seed=1000)
    b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"], device=dev)
    ids, ln = gtok.ops.sent(b, maxn, 1024, 3, 2, labeled=True, num_node_types=28, num_edge_types=4)
    got, st = gtok.ops.sent_decode_csr(ids, ln, maxn, True, 28)
    whole = bool((st == 0).all()) and (got.num_nodes_total, got.num_edges_total) == (b.num_nodes_total, b.num_edges_total)
    phases = {}
    for _ in range(REPEATS):
        tsd.new_route(gtok, torch, ids, ln, maxn, True, 28, phases=phases)
    return dict(rows=int(ids.shape[0]), ld=int(ids.shape[1]), equal=whole, phases={k: med(v) for k, v in phases.items()})


def phases_of(job: str, res: dict) -> dict:
    if job.startswith("ibtt:"):
        return {"gtok_ibtt_decode_sizes": res["ms"]["sizes"][0], "gtok_ibtt_decode_csr": res["ms"]["csr"][0]}
    p = res["phases"]["new"] if job.startswith("sent:") else res["phases"]
    return {k: p[k] for k in ("gtok_sent_decode_sizes", "gtok_sent_decode_csr")}


def run_job(job: str, parent_lib: str, out_dir: str) -> None:
    tool, _, shape = job.partition(":")
    cmd = {"sent": [os.path.join(HERE, "time_sent_decode_csr.py"), "--child", shape], "ibtt": [os.path.join(HERE, "time_ibtt_decode.py"), "--child", shape],
           "twice": [os.path.abspath(__file__), "--child"]}[tool]
    sides = {"parent": [], "branch": []}
    for i in range(PROCS):
        for side in (("parent", "branch") if i % 2 == 0 else ("branch", "parent")):
            env = {k: v for k, v in os.environ.items() if k != "GTOK_LIB"}
            if side == "parent":
                env["GTOK_LIB"] = os.path.abspath(parent_lib)
            t0 = time.perf_counter()
            p = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable] + cmd, capture_output=True, text=True, env=env)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-4000:])
                sys.exit(f"{job}: process {i} of the {side}'s library ended with status {p.returncode}: stopping")
            res = json.loads(line[0][7:])
            if res.get("equal", res.get("equal_on_sample")) is not True:
                sys.exit(f"{job}: process {i} of the {side}'s library: the routes' results differ: stopping")
            sides[side].append(phases_of(job, res))
            print(job, i, side, sides[side][-1], f"({time.perf_counter() - t0:.0f} s)", flush=True)
            with open(os.path.join(out_dir, "ab_" + job.replace(":", "_") + ".json"), "w") as f:
                json.dump(sides, f, indent=1)


def report(out_dir: str) -> int:
    lines = ["# The decoders' kernels on the parent's build and on this one: timing", "",
             "`python profiles/tools/ab_time_decode.py PARENT_LIB OUT_DIR` (PARENT_LIB from `profiles/tools/ab_build.sh <parent> parent`).  Wall time around a "
             "device synchronise, ms per call of the entry point alone.  Per job and side three or more fresh processes, the two libraries alternating in "
             "who goes first; a process reports the median of each phase; a cell lists the processes' medians, then their median.  Margin: this build's "
             "median may exceed the parent's by no more than the parent's spread (largest - smallest of its processes' medians).", "",
             "| job | phase | parent, ms | this build, ms | parent's spread, ms | this build - parent, ms | verdict |", "|---|---|---|---|---|---|---|"]
    failed = 0
    for job in JOBS:
        path = os.path.join(out_dir, "ab_" + job.replace(":", "_") + ".json")
        if not os.path.exists(path):
            continue
        sides = json.load(open(path))
        for ph in sides["parent"][0]:
            a, b = [r[ph] for r in sides["parent"]], [r[ph] for r in sides["branch"]]
            spread, excess = max(a) - min(a), med(b) - med(a)
            ok = len(a) >= 3 and len(b) >= 3 and excess <= spread
            failed += not ok
            cell = lambda v: ", ".join(f"{x:.3f}" for x in v) + f": {med(v):.3f}"
            lines.append(f"| {job} | {ph} | {cell(a)} | {cell(b)} | {spread:.3f} | {excess:+.3f} | {'within' if ok else 'SLOWER'} |")
    with open(os.path.join(out_dir, "timing.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if failed else 0


def main():
    if len(sys.argv) >= 2 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(twice_child()))
        return 0
    if len(sys.argv) == 3 and sys.argv[1] == "--report":
        return report(sys.argv[2])
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    parent_lib, out_dir = sys.argv[1], sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    for job in sys.argv[3:] or JOBS:
        run_job(job, parent_lib, out_dir)
    return report(out_dir)


if __name__ == "__main__":
    sys.exit(main())
