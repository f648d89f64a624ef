"""The bench line committed under profiles/ (the last `python bench.py` run of the round on an MI355X; every leg it
holds now comes with `--full`) against the driver's contract: required keys, the `roofline` and `cpu_baseline`
objects, internal consistency, and the metric of BASELINE.json.  A schema regression in bench.py shows up here on the
CPU, not at round end.  `--dump-outputs` and the plain run's line are checked below."""

import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(name):
    with open(os.path.join(ROOT, "profiles", "r03", name)) as fh:
        rows = [l for l in fh.read().splitlines() if l.startswith("{")]
    assert len(rows) == 1, "exactly one JSON line"
    return json.loads(rows[0])


def test_default_line_follows_the_contract():
    d = _line("bench_n1.json")
    with open(os.path.join(ROOT, "BASELINE.json")) as fh:
        base = json.load(fh)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and base["metric"].startswith(d["metric"])      # BASELINE.json's headline metric
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["scaling"] in ("weak", "strong")
    assert "workload" in d["config"] and "model" not in d["config"]
    # value = frames of the job / step time
    frames = d["config"]["frames_total"]
    assert abs(d["value"] - frames / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    # achieved = algorithmic bytes (24 N + 72 per frame) / the live launch duration
    n = d["config"]["n_atoms"]
    assert r["algorithmic_bytes"] == r["frames_in_launch"] * (24 * n + 72)
    assert abs(r["achieved"] - r["algorithmic_bytes"] / r["launch_seconds"] / 1e9) / r["achieved"] < 1e-9
    assert r["launch_seconds"] * 1e3 <= d["ms_per_step"]            # the dominant kernel fits inside a step
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["unit"] == d["unit"]
    assert d["verified"] is True and d["verification"]["ok"] is True


def test_two_rank_rehearsal_line():
    d = _line("bench_2rank_rehearsal.json")
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["verified"] is True
    assert d["config"]["trajectory_identical_on_all_ranks"] is True
    ranks = d["per_rank"]
    assert [r["rank"] for r in ranks] == [0, 1]
    # the two ranks' frame shards tile the trajectory
    assert ranks[0]["rdf_frames"][0] == 0 and ranks[0]["rdf_frames"][1] == ranks[1]["rdf_frames"][0]
    assert ranks[1]["rdf_frames"][1] == d["config"]["frames_total"]


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus N` from a plain shell (the shape of the driver's command): the parent starts the ranks
    as a child process through torch.distributed.run on 127.0.0.1, relays their output and their exit code.  Checked
    here without a GPU through --rank-probe (every rank reports RANK / WORLD_SIZE and exits before touching torch)."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    bench = os.path.join(ROOT, "bench.py")
    ok = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "1", "--rank-probe", "0"], env=env,
                        capture_output=True, text=True, timeout=300)
    assert ok.returncode == 0, ok.stderr[-2000:]
    probes = [json.loads(l) for l in ok.stdout.splitlines() if l.startswith("{")]
    assert sorted(p["rank"] for p in probes) == [0, 1]
    assert all(p["world"] == 2 and p["gpus"] == 2 and p["master_addr"] == "127.0.0.1" for p in probes)
    bad = subprocess.run([sys.executable, bench, "--gpus", "2", "--rank-probe", "3"], env=env, capture_output=True,
                         text=True, timeout=300)
    assert bad.returncode != 0                      # a failing rank is not swallowed by the launcher
    # under a launcher with a different world size the mismatch is an error, not a silent single-rank run
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    one = subprocess.run([sys.executable, bench, "--gpus", "1", "--rank-probe", "0"], env=env2, capture_output=True,
                         text=True, timeout=300)
    assert one.returncode == 0 and json.loads(one.stdout.strip())["world"] == 1


def _fake_results(bins=300, windows=7):
    import types
    import pandas as pd
    rng = np.random.default_rng(5)
    rdf = types.SimpleNamespace(data=pd.DataFrame({"r": np.arange(bins) * 0.01, "X": rng.random(bins)}),
                                hist=rng.integers(0, 1 << 40, (4, 4, bins)).astype(np.uint64))
    msd = types.SimpleNamespace(data=pd.DataFrame({"Time": np.arange(windows) * 100, "Zn": rng.random(windows)}),
                                sumsq=rng.random((4, windows)))
    return rdf, msd


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    import bench
    rdf, msd = _fake_results()
    bench.dump_outputs(str(tmp_path), rdf, msd)
    got = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("rdf_data", "rdf_hist", "msd_data", "msd_sumsq")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["rdf_data"], rdf.data.to_numpy(dtype=np.float64))
    assert np.array_equal(got["rdf_hist"].astype(np.uint64), rdf.hist)            # counts below 2^53 are exact
    assert np.array_equal(got["msd_data"], msd.data.to_numpy(dtype=np.float64))
    assert np.array_equal(got["msd_sumsq"], msd.sumsq)


def test_dump_outputs_samples_the_same_elements_beyond_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4096)
    rdf, msd = _fake_results()
    bench.dump_outputs(str(tmp_path / "a"), rdf, msd)
    bench.dump_outputs(str(tmp_path / "b"), rdf, msd)
    total = 0
    for name in ("rdf_data", "rdf_hist", "msd_data", "msd_sumsq"):
        a, b = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert a.dtype == np.float64 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 4096
    assert set(np.load(str(tmp_path / "a" / "rdf_hist.npy")).tolist()) <= set(rdf.hist.reshape(-1).astype(np.float64).tolist())


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    """A run without --full prints the headline line and nothing measured beside it; --dump-outputs holds the results
    of the last timed step, which the same seeded trajectory through the same classes reproduces in this process."""
    import subprocess
    import sys
    import torch
    from amof_amd.rdf import Rdf
    from amof_amd.msd import WindowMsd
    from tests import helpers as H
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out_dir = tmp_path / "outputs"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", "400", "--steps", "2",
                          "--warmup", "1", "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    rows = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(rows) == 1
    d = rows[0]
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["config"]["frames_total"] == 400
    assert abs(d["value"] - 400 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert d["verified"] is None
    for k in ("configs3", "roofline_msd", "verification", "cpu_baseline", "cn_headline", "realistic_cells", "supplementary"):
        assert k not in d, k
    packed = H.device_walk(torch.device("cuda", 0), (3, 3, 4), 400, 0.05, 20261003)
    torch.cuda.synchronize()
    rdf = Rdf.from_trajectory(packed, device=0, distributed=False)
    msd = WindowMsd.from_trajectory(packed, delta_time=100, timestep=1, device=0, distributed=False)
    got = {n: np.load(str(out_dir / (n + ".npy"))) for n in ("rdf_data", "rdf_hist", "msd_data", "msd_sumsq")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["rdf_hist"], np.asarray(rdf.hist).view(np.uint64).astype(np.float64))
    assert np.array_equal(got["rdf_data"], rdf.data.to_numpy(dtype=np.float64))
    assert got["msd_data"].shape == (len(msd.data), len(msd.data.columns)) and len(msd.data) == 2
    np.testing.assert_allclose(got["msd_data"], msd.data.to_numpy(dtype=np.float64), rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got["msd_sumsq"], np.asarray(msd.sumsq), rtol=1e-12, atol=0.0)
