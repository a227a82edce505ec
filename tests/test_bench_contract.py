"""The contract of bench.py's output line (what the driver parses): exactly one line on stdout, the fields of the task's
schema, the roofline and cpu_baseline objects of --full, and the consistency the numbers must have among themselves; a plain
run times exactly --steps steps and --dump-outputs writes what those steps returned."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_fields_and_consistency():
    d = _run(["--full", "--steps", "16", "--warmup", "4", "--repeats", "6", "--cpu-sample-envs", "16"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "repeats", "preroll_steps"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 16 and d["warmup"] == 4 and d["repeats"] == 6 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and "workload" in d["config"] and "model" not in d["config"]
    B = d["config"]["global_batch"]
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6          # value = batch / time per batch step
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is not None and r["traffic"] > 0 and r["issue_bound"]["peak"] == 1.0
    assert 0 < r["kernel_ms_per_launch"] <= d["ms_per_step"] * d["steps"] * 1.05          # the kernel is inside the timed launch
    # the HBM figure is the one SURVEY 8d prescribes; the line also says what really binds, and which kernel the counters are of
    assert r["binding"] == "issue" and r["traffic_kernel"] and isinstance(r["traffic_kernel_is_timed_kernel"], bool)
    assert r["issue_bound"]["kernel"] == r["traffic_kernel"]
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] == 1 and c["value"] > 0 and c["additions_match_device"] is True
    ca = d["cpu_baseline_all_cores"]                                                       # one environment stream per host core
    assert ca["kind"] == c["kind"] and ca["cores"] >= 1 and ca["threads"] == ca["cores"] and ca["nproc"] >= ca["cores"] and ca["value"] > 0
    assert ca["additions_match_device"] in (True, None)
    ss = d["session_stats"]                                                                # the sustained figure's evidence: nothing left the class
    assert set(ss["timed_region"]) == {"sessions", "joined", "later_kernel_steps", "kernels", "spills"} and ss["timed_region"]["spills"] >= 0
    assert d["long_launch"]["launches"] >= 8 and d["long_launch"]["value"] > 0 and d["rehearsal"] is False


@pytest.mark.gpu
def test_bench_spawns_its_ranks_and_prints_one_line():
    d = _run(["--full", "--gpus", "2", "--steps", "8", "--warmup", "2", "--repeats", "4", "--no-cpu-baseline", "--allow-oversubscribe"])   # two ranks on the one device
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 2 * 4096 and d["value"] > 0
    assert d["oversubscribed"] is True and len(d["per_rank_value"]) == 2 and all(v > 0 for v in d["per_rank_value"])


def _rehearse(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rehearse-plumbing", "--batch", "64"] + args, cwd=ROOT,
                          capture_output=True, text=True, timeout=600, env=env)


def test_plain_run_times_exactly_the_steps_asked_for():
    """Without --full the timed region is one launch of --steps steps and nothing but the headline is measured (rehearsed:
    the stand-in counts the steps issued to it)."""
    p = _rehearse(["--steps", "37", "--warmup", "3"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 37 and d["repeats"] == 1 and d["timed_steps"] == 37 and d["full"] is False
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["long_launch"] is None


def test_plain_run_refuses_what_needs_full_or_a_device(tmp_path):
    p = _rehearse(["--steps", "4", "--repeats", "0"])
    assert p.returncode != 0 and "needs --full" in p.stderr and not p.stdout.strip()
    p = _rehearse(["--steps", "4", "--dump-outputs", str(tmp_path / "out")])
    assert p.returncode != 0 and "needs the device" in p.stderr and not p.stdout.strip()
    assert not (tmp_path / "out").exists()


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run: the headline fields, exactly --steps timed steps, nothing of --full; --dump-outputs writes the timed
    launch's last outputs (float32 / float64, <= 64 MB), and a second run with the same arguments writes the same arrays."""
    import numpy as np
    runs = []
    for i in range(2):
        out = tmp_path / ("run%d" % i)
        d = _run(["--steps", "64", "--warmup", "8", "--dump-outputs", str(out)])
        runs.append((d, out))
    d = runs[0][0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["full"] is False
    assert d["steps"] == 64 and d["warmup"] == 8 and d["repeats"] == 1 and d["timed_steps"] == 64
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["long_launch"] is None
    B = d["config"]["global_batch"]
    assert d["value"] > 0 and abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    names = sorted(f.name for f in runs[0][1].iterdir())
    assert names == ["dones.npy", "obs.npy", "obs_env_ids.npy", "rewards.npy", "rows.npy"], names
    assert sum(f.stat().st_size for f in runs[0][1].iterdir()) <= 64 << 20
    a = {n: np.load(runs[0][1] / n) for n in names}
    b = {n: np.load(runs[1][1] / n) for n in names}
    for n in names:
        assert a[n].dtype in (np.float32, np.float64), (n, a[n].dtype)
        assert a[n].shape == b[n].shape and np.array_equal(a[n], b[n]), n
    rows, obs, ids = a["rows.npy"], a["obs.npy"], a["obs_env_ids.npy"].astype(np.int64)
    assert rows.shape == (B,) and a["rewards.npy"].shape == (B,) and set(np.unique(a["dones.npy"])) <= {0.0, 1.0}
    assert obs.shape[0] == len(ids) and obs.shape[1] == max(1, int(rows.max())) and 0 <= rows.min() and rows.max() <= 512
    live = np.arange(obs.shape[1])[None, :] < rows[ids, None]
    assert (obs[~live] == -1).all() and (obs[live] >= 0).all()
