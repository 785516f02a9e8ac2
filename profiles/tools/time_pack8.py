"""The walk that packs 8-bit rows against the walk that packs 16-bit rows, this build against the build of an earlier git ref
(HIP events; ZINC-full shape: 249,456 molecules, K = 16 epochs per launch, pack-only).

    python profiles/tools/time_pack8.py OUT_DIR [PARENT_LIB]

The driver starts worker processes in pairs - one with this tree's libgtok.so, one with PARENT_LIB (built from the parent
commit, profiles/tools/ab_build.sh) loaded through GTOK_LIB in a process of its own - lets both set up, and then ALTERNATES
them: one repeat = a warm-up and LAUNCHES launches between two events, REPEATS repeats per leg and pair, PROCS pairs, parent
and branch in turn, so that drift of the machine hits both alike.  Medians and min-max spreads over all of a leg's repeats go to
OUT_DIR/time_pack8.json (copy it to profiles/rows8/).  Reported without a threshold: gtok_pack_rows_scan 2 -> 1 byte against 2 -> 2 on the same slab, and the
one-rank nccl rehearsal of dist.gather_tokens (pre-packed rows, left packed) at 8 and 16 bits: bytes handed to the collective
and time.  That rehearsal is ONE rank: no multi-GPU run exists for this project and nothing here is a scaling result."""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G, LD, K = int(os.environ.get("G", 249456)), 176, int(os.environ.get("K", 16))
REPEATS, LAUNCHES, WARMUP = int(os.environ.get("REPEATS", 3)), int(os.environ.get("LAUNCHES", 100)), 10
PROCS = int(os.environ.get("PROCS", 5))         # fresh worker processes per library


def worker():
    import torch
    sys.path.insert(0, ROOT)
    gtok = importlib.import_module("glearning-benchmark_amd")
    dev = torch.device("cuda:0")
    d = gtok.synth.zinc_like(G, seed=1000)
    b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"], device=dev)
    kw = dict(labeled=True, num_node_types=9, num_edge_types=4, remap_zinc=True)
    version = gtok._lib.library_version()
    ln = torch.empty(K * G, dtype=torch.int32, device=dev)
    _, ln0 = gtok.ops.sent(b, 37, 1024, 0, 0, ld=LD, pad=False, epochs=K, u16=True, **kw)
    n = ln0.reshape(-1).clamp(0, LD).long()
    need = {2: int(((n + 7) // 8 * 8).sum()), 1: int(((n + 15) // 16 * 16).sum())}
    del ln0
    pks = {2: gtok.ops.PackedRows(K * G, int(need[2] * 1.04) + 4096, True, dev)}
    if version >= 8:
        pks[1] = gtok.ops.PackedRows(K * G, int(need[1] * 1.04) + 4096, True, dev, elem_bytes=1)

    def timed(f, launches=LAUNCHES, warmup=WARMUP):
        for _ in range(warmup):
            f()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(launches):
            f()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / launches

    def walk(eb):
        pk = pks[eb]
        return lambda: gtok.ops.sent(b, 37, 1024, 0, 0, ld=LD, epochs=K, u16=True, packed=pk, slab=False, out=(None, ln), check_ids=False, **kw)

    print(json.dumps(dict(ready=True, version=version, need=need)), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        if cmd in ("walk16", "walk8"):
            eb = 2 if cmd == "walk16" else 1
            ms = timed(walk(eb))
            pk = pks[eb]
            out = dict(ms=ms, used=int(pk.used()), status=int(pk.status()), fused=bool(pk.fused), payload_bytes=int(pk.used()) * eb)
        elif cmd == "scan":          # the one-pass pack of ONE epoch's 16-bit slab at 2 and at 1 byte per id
            slab, sl = gtok.ops.sent(b, 37, 1024, 0, 0, ld=LD, pad=False, u16=True, **kw)
            out = {}
            for eb, al in ((2, 8), (1, 16)):
                cap = int((((sl.clamp(0, LD).long() + al - 1) // al) * al).sum())
                f = lambda: gtok.ops.pack_rows_scan(slab, sl, eb, cap, align=al)
                out[f"scan_2_to_{eb}_ms"] = sorted(timed(f, 200) for _ in range(5))
                out[f"scan_2_to_{eb}_bytes"] = cap * eb
                assert int(f()[2].item()) == 0
            del slab
        elif cmd == "nccl":          # one rank: the collective runs, nothing is learnt about links
            import socket
            import torch.distributed as tdist
            s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            tdist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
            out = {}
            try:
                for eb in (2, 1):
                    walk(eb)()
                    st = {}
                    f = lambda: gtok.dist.gather_tokens(None, ln, K * G, 5, force=True, compact=True, packed=pks[eb], ld=LD, as_packed=True, stats=st)
                    out[f"gather_{8 * eb}bit_ms"] = sorted(timed(f, 20, 3) for _ in range(5))
                    out[f"gather_{8 * eb}bit_bytes_sent_per_rank"] = st["bytes_sent_per_rank"]
                    out[f"gather_{8 * eb}bit_packed_bytes"] = st["capacity"] * st["elem_bytes"]
            finally:
                tdist.destroy_process_group()
        else:
            out = dict(error=cmd)
        print(json.dumps(out), flush=True)


class Worker:
    def __init__(self, lib):
        env = dict(os.environ)
        if lib:
            env["GTOK_LIB"] = lib
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=env, text=True)
        self.hello = self.read()

    def read(self):
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"worker ended (exit status {self.p.poll()})")
            if line.startswith("{"):
                return json.loads(line)

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n"); self.p.stdin.flush()
        return self.read()

    def close(self):
        try:
            self.p.stdin.write("quit\n"); self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def summary(ts):
    ts = sorted(ts)
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], spread_ms=ts[-1] - ts[0], repeats=ts)


def main():
    out_dir = sys.argv[1]
    parent_lib = sys.argv[2] if len(sys.argv) > 2 else None
    os.makedirs(out_dir, exist_ok=True)
    res = dict(shape=dict(G=G, K=K, ld=LD, launches_per_repeat=LAUNCHES, warmup=WARMUP, repeats_per_process=REPEATS, processes_per_library=PROCS))
    legs = dict(branch_walk8=[], branch_walk16=[])
    if parent_lib:
        legs["parent_walk16"] = []
    info, paired = {}, []
    # A process keeps its level: two processes of ONE library differ by up to 6 % (0.96 against 1.03 ms, whichever starts first),
    # repeats inside a process by 0.3 %.  So every library gets PROCS fresh processes, a parent and a branch process alive side by
    # side and asked in turn; the spread over ALL of a leg's repeats is the run-to-run spread, and the difference between the two
    # widths is also taken inside each branch process, where that level cancels.
    for proc in range(PROCS):
        first_parent = bool(parent_lib) and proc % 2 == 1
        parent = Worker(parent_lib) if first_parent else None
        branch = Worker(None)
        if parent_lib and not first_parent:
            parent = Worker(parent_lib)
        try:
            res["branch_abi"], res["need_ids"] = branch.hello["version"], branch.hello["need"]
            if parent:
                res["parent_abi"] = parent.hello["version"]
            mine = {name: [] for name in legs}
            for rep in range(REPEATS):           # parent and branch in turn, the order of the legs turning with the repeats
                names = list(legs)
                for name in names[(rep + proc) % len(names):] + names[:(rep + proc) % len(names)]:
                    w = parent if name.startswith("parent") else branch
                    r = w.ask("walk8" if name.endswith("8") else "walk16")
                    mine[name].append(r.pop("ms"))
                    info[name] = r
            for name in legs:
                legs[name] += mine[name]
            med = lambda ts: sorted(ts)[len(ts) // 2]
            paired.append(med(mine["branch_walk8"]) - med(mine["branch_walk16"]))
            if proc == PROCS - 1:
                res["pack_rows_scan"] = branch.ask("scan")
                res["one_rank_nccl_rehearsal"] = branch.ask("nccl")
        finally:
            branch.close()
            if parent:
                parent.close()
    for name, ts in legs.items():
        res[name] = dict(summary(ts), **info[name])
    res["walk8_minus_walk16_ms_inside_each_branch_process"] = paired
    if parent_lib:
        p = res["parent_walk16"]
        bound = p["median_ms"] + p["spread_ms"]
        res["bound_ms"] = bound
        res["walk8_no_slower_than_parent_walk16"] = res["branch_walk8"]["median_ms"] <= bound
        res["walk16_no_slower_than_parent_walk16"] = res["branch_walk16"]["median_ms"] <= bound
    res["payload_ratio_8_over_16"] = res["branch_walk8"]["payload_bytes"] / res["branch_walk16"]["payload_bytes"]
    with open(os.path.join(out_dir, "time_pack8.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    for k in ("parent_walk16", "branch_walk16", "branch_walk8"):
        if k in res:
            print(k, {a: round(res[k][a], 5) for a in ("median_ms", "min_ms", "max_ms")})


if __name__ == "__main__":
    worker() if "--worker" in sys.argv else main()
