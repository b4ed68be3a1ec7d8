"""bench.py --gpus N starts N ranks itself (the driver's N-GPU command): the launcher's
children see torch.distributed.run's environment (RANK, LOCAL_RANK, WORLD_SIZE,
MASTER_ADDR=127.0.0.1) and form one process group of world size N (gloo on CPU here;
RCCL on the GPU box)."""
import json
import os
import sys

import bench

HERE = os.path.dirname(os.path.abspath(__file__))


def test_launcher_forms_world_of_two(tmp_path):
    out = str(tmp_path / "probe")
    rc = bench.launch_ranks(2, script=os.path.join(HERE, "helpers", "rank_probe.py"), argv=["2", out])
    assert rc == 0
    got = [json.load(open("%s.%d" % (out, r))) for r in range(2)]
    assert [g["rank"] for g in got] == [0, 1]
    assert all(g["world"] == 2 and g["sum"] == 3 for g in got)


def test_configs_cover_baseline():
    """Every BASELINE.json GPU config has a bench workload (C2 default)."""
    cfg = json.load(open(os.path.join(os.path.dirname(HERE), "BASELINE.json")))["configs"]
    assert len(cfg) == 5 and set(bench.CONFIGS) == {"C2", "C3", "C4", "C5"}
    assert bench.CONFIGS["C2"]["games"] == 4096 and bench.CONFIGS["C2"]["visits"] == 600
    assert (bench.CONFIGS["C5"]["X"], bench.CONFIGS["C5"]["arch"]) == (9, "b18c384nbt")


def test_plain_run_measures_the_headline_window_only(monkeypatch):
    """Without --full: no CPU baseline, no second or trained-net window; --full restores them
    (and the switches that narrow a full run still apply)."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 2, False, None)
    assert a.no_cpu_baseline and not a.compliant_line and a.trained_steps == 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert not a.no_cpu_baseline and a.compliant_line and a.trained_steps == 200
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--config", "C3", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.no_cpu_baseline and a.trained_steps == 0 and a.precision == "default"


def test_dump_outputs_orders_and_samples_rows(tmp_path, monkeypatch):
    """--dump-outputs: float32 copies of every row field in (slot, game, turn) order whatever
    order the rows arrived in; above the size bound the same seeded sample every time."""
    import numpy as np
    from katacoffee_amd import rows as kcrows
    X = Y = 5
    n = 200
    rng = np.random.default_rng(1)
    sh = kcrows.shapes(X, Y)
    rows = {f: rng.integers(0, 100, (n,) + sh[f]).astype(t) for f, t in kcrows.FIELDS}
    rows["meta"][:, 0] = np.arange(n) // 10
    rows["meta"][:, 1] = np.arange(n) % 10 // 5
    rows["meta"][:, 2] = np.arange(n) % 5
    perm = rng.permutation(n)
    counters = {"moves": 7, "playouts": 1 << 40, "nn_evals": 9}
    bench.dump_outputs(str(tmp_path / "a"), {f: a[perm] for f, a in rows.items()}, counters, seed=3)
    for f, _ in kcrows.FIELDS:
        got = np.load(tmp_path / "a" / (f + ".npy"))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, rows[f].astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "counters.npy"), [n, n, 7, float(1 << 40), 9])
    per_row = 4 * sum(int(np.prod(s)) for s in sh.values())
    monkeypatch.setattr(bench, "DUMP_BYTES", 50 * per_row)
    for d, p in (("b", perm), ("c", rng.permutation(n))):
        bench.dump_outputs(str(tmp_path / d), {f: a[p] for f, a in rows.items()}, counters, seed=3)
    meta = np.load(tmp_path / "b" / "meta.npy")
    assert meta.shape == (50, 4) and [tuple(m) for m in meta[:, :3]] == sorted(tuple(m) for m in meta[:, :3])
    for f, _ in kcrows.FIELDS:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / (f + ".npy")), np.load(tmp_path / "c" / (f + ".npy")))
    assert sum(os.path.getsize(tmp_path / "b" / x) for x in os.listdir(tmp_path / "b")) <= 50 * per_row + 8 * 200
