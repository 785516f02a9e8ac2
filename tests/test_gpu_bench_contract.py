"""GPU: `python bench.py` keeps the driver's contract - one JSON line on stdout with the agreed keys; with --full the
`roofline` and `cpu_baseline` objects and a CPU sample that matched the GPU's ids; --dump-outputs writes the last timed
step's rows."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_contract_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "zinc_subset", "--steps", "3",
                        "--warmup", "1", "--cpu-sample", "2000", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    b = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in b, k
    assert b["n_gpus"] == 1 and b["steps"] == 3 and b["warmup"] == 1 and b["higher_is_better"] is True
    assert b["scaling"] == "weak" and b["vs_baseline"] is None and b["data"] == "synthetic" and b["dtype"] == "int32"
    assert isinstance(b["config"].get("workload"), str) and "model" not in b["config"]
    assert b["value"] > 0 and b["ms_per_step"] > 0
    rf = b["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(rf) and rf["bound"] == "hbm"
    assert rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    cb = b["cpu_baseline"]
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(cb) and cb["kind"] in ("port", "reference")
    assert cb["cores"] >= 1 and cb["value"] > 0 and cb.get("parity_with_gpu") is True
    # round 4: a step is an epoch, a launch carries E of them for the split that cannot fill the chip on its own
    assert b["config"]["epochs_per_launch"] == 3 and rf["epochs_per_launch"] == 3 and rf["launches"] == 1
    assert "cold_start" in b and b["cold_start"]["ms_per_step"] > 0 and "u16_rows" in b


def test_truncation_aware_yardstick_counts_the_nodes_the_walks_reach():
    """the decode pass behind roofline.truncation_aware stopped at its capacities (~5 nodes per walk reported
    where the walks reach ~68).  The count-only decode reads every row to its end."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "synth_er", "--graphs", "24000", "--steps", "3",
                        "--warmup", "1", "--no-cpu-baseline", "--no-ibtt", "--no-sustained", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    b = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][0])
    ta = b["roofline"]["truncation_aware"]
    assert ta["avg_nodes_visited"] > 30, ta
    assert 0 < ta["bytes_per_launch"] <= b["roofline"]["algorithmic_bytes_per_launch"]


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """A plain run (no --full) prints the headline line without the secondary legs, and --dump-outputs writes what the
    last of the K timed steps computed: here epoch W + K - 1, slice K - 1 of one 5-epoch launch, against the CPU oracle."""
    import numpy as np
    from _util import gtok, orc
    steps, warmup = 5, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "zinc_subset", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    b = json.loads(lines[0])
    assert b["metric"] == "graphs_tokenized_per_sec" and b["unit"] == "graphs/s" and b["dtype"] == "int32" and b["higher_is_better"] is True
    assert b["steps"] == steps and b["value"] > 0 and b["ms_per_step"] > 0 and b["config"]["epochs_per_launch"] == steps
    assert not {"cpu_baseline", "cold_start", "u16_rows", "epoch_loop", "ibtt", "boundary"} & set(b)
    ids, ln, rows = (np.load(tmp_path / f"{n}.npy") for n in ("sent_ids", "sent_lengths", "sent_rows"))
    assert ids.dtype == ln.dtype == np.float32 and rows.dtype == np.float64
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20
    d = gtok.synth.zinc_like(12000, seed=1000)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"])
    assert ids.shape == (12000, b["config"]["slab_width"]) and np.array_equal(rows, np.arange(12000))
    ref, rln = orc.sent(coo, int(d["node_counts"].max()), 1024, 0, warmup + steps - 1, labeled=True, num_node_types=9,
                        num_edge_types=4, remap_zinc=True, ld=ids.shape[1], nthreads=8)
    assert np.array_equal(ln, rln) and np.array_equal(ids, ref)
