"""bench.py's host logic that needs no GPU: the `other_configs` pass (BASELINE configs[2..4]
measured by child processes of the script and embedded in the headline line) keeps what it reads
to the fields the line is read for and turns a failing child into an `error` entry."""
import importlib.util
import json
import os
import subprocess
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_other_configs_pass_summarises_children_and_survives_failures(monkeypatch):
    bench = load_bench()
    calls = []

    def fake_run(cmd, **kw):
        calls.append(cmd)
        # the children keep their CPU leg (the reference binary on one core rides in every entry)
        assert "--no-cpu-baseline" not in cmd and kw.get("timeout", 0) <= 300
        if "lm" in cmd and "cholesky" in cmd:
            return types.SimpleNamespace(returncode=1, stdout="", stderr="boom: no GPU here")
        line = {"metric": "m", "value": 2.5, "unit": "u/s", "steps": 7, "ms_per_step": 0.4, "dtype": "f64",
                "config": {"workload": "w", "solver": "qr", "whole_run": {"value": 3.0},
                           "reference_order": {"value": 1.5}, "other_solver": {"solver": "qr", "value": 1.0, "ms_per_step": 2.0,
                                                            "extra": "dropped"}},
                "roofline": {"bound": "hbm", "achieved": 1.0, "peak": 2.0, "unit": "GB/s", "frac": 0.5,
                             "kernel": "k", "kernel_ms": 0.1, "traffic": 123, "noise": "dropped"},
                "cpu_baseline": {"value": 9}}
        return types.SimpleNamespace(returncode=0, stdout="banner\n" + json.dumps(line) + "\n", stderr="")

    monkeypatch.setattr(subprocess, "run", fake_run)
    out = bench.other_configs_pass()
    assert len(out) == len(calls) >= 4
    ok = [e for e in out if "error" not in e]
    bad = [e for e in out if "error" in e]
    assert len(bad) == 1 and "rc=1" in bad[0]["error"] and "boom" in bad[0]["error"]
    for e in ok:
        assert e["value"] == 2.5 and e["workload"] == "w" and e["roofline"]["frac"] == 0.5
        assert "noise" not in e["roofline"] and e["cpu_baseline"] == {"value": 9}
        assert e["other_solver"] == {"solver": "qr", "value": 1.0, "ms_per_step": 2.0}
        # every entry states whether its dominant kernel fits into its step (0.1 <= 0.4 here)
        assert e["kernel_within_step"] is True and e["solver"] == "qr" and e["whole_run"] == {"value": 3.0}
        assert e["reference_order"] == {"value": 1.5}  # the same workload in the other summation order
    assert all(e["config"].startswith(("configs[", "north_star", "SURVEY")) for e in out)
    # the default-functor workloads (reference order) ride along
    assert any("bfgs-fd" in c for c in calls) and any("lm-fd" in c for c in calls)
    # BASELINE words configs[3] with the tinyqr solve: that solver is an entry of its own, and it
    # comes before the Cholesky one
    lm = [c for c in calls if "lm" in c and "--lm-n" not in c]
    assert len(lm) == 2 and "qr" in lm[0] and "cholesky" in lm[1]
    # the sizes past the one-wave kernels and the tinyqr surface are measured in the same line
    assert any("--lm-n" in c and "128" in c for c in calls) and any("tinyqr" in c for c in calls)
    assert any("tinyqr" in e["config"] for e in out)


def test_kernel_within_step_check_records_and_never_raises():
    """A violation must not cost the JSON line: it is recorded (the line carries
    kernel_within_step = false) and turns into a non-zero exit only after the line is out."""
    bench = load_bench()
    assert bench.check_kernel_within_step(0.50, 0.51, "x") is True
    assert bench.check_kernel_within_step(0.515, 0.51, "x") is True  # timer noise
    assert bench.CONSISTENCY_VIOLATIONS == []
    assert bench.check_kernel_within_step(16.2, 13.4, "bfgs") is False
    assert len(bench.CONSISTENCY_VIOLATIONS) == 1 and "different regimes" in bench.CONSISTENCY_VIOLATIONS[0]


def test_timed_region_is_repeated_until_it_covers_the_minimum():
    bench = load_bench()
    import time as _t

    class Ranks:
        def barrier(self):
            pass

        def max_over_ranks(self, v):
            return v

    calls = []

    def stepper(n):
        calls.append(n)
        _t.sleep(0.0005 * n)

    dt, done = bench.timed_steps(Ranks(), stepper, 20)  # 10 ms per 20 steps -> repeated to >= 50 ms
    assert calls[0] == 20 and len(calls) == 2 and done == sum(calls) and done >= 80
    assert dt >= bench.MIN_TIMED_S * 0.9
    calls.clear()
    dt, done = bench.timed_steps(Ranks(), stepper, 200)  # already 100 ms
    assert calls == [200] and done == 200
    calls.clear()
    dt, done = bench.timed_steps(Ranks(), stepper, 20, min_s=0.0)  # the headline: exactly 20 steps
    assert calls == [20] and done == 20


def test_dump_outputs_writes_float64_within_budget(tmp_path, monkeypatch):
    """--dump-outputs writes what the timed path leaves a caller as float64 .npy files: every
    score, the best agent, the status and a fixed, seeded sample of population rows, which is the
    same on every call and keeps the files under 64 MB at any population size."""
    import numpy as np
    bench = load_bench()

    class Eng:
        def best(self):
            return np.arange(4.0), -1.5, 7

    st = types.SimpleNamespace(iteration=12, function_calls_used=13 * 20000, std_err=0.25)
    n = 20000
    population = np.arange(n * 4, dtype=np.float64).reshape(n, 4)
    scores = np.arange(n, dtype=np.float64)
    bench.dump_de_outputs(str(tmp_path / "a"), Eng(), st, population, scores)
    got = {f.stem: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["best_x", "population_sample", "scores", "status"]
    assert all(a.dtype == np.float64 for a in got.values())
    rows = bench.dump_rows(n)
    assert len(rows) == bench.DUMP_POP_ROWS and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.array_equal(rows, bench.dump_rows(n))
    assert np.array_equal(got["population_sample"], population[rows])
    assert np.array_equal(got["scores"], scores) and np.array_equal(got["best_x"], np.arange(4.0))
    assert got["status"].tolist() == [-1.5, 7, 12, 13 * 20000, 0.25]
    assert np.array_equal(bench.dump_rows(100), np.arange(100))
    assert bench.DUMP_POP_ROWS * bench.D * 8 + bench.DUMP_SCORES_MAX * 8 <= 64e6
    # past DUMP_SCORES_MAX agents the scores are cut to the same row sample
    monkeypatch.setattr(bench, "DUMP_SCORES_MAX", n - 1)
    bench.dump_de_outputs(str(tmp_path / "b"), Eng(), st, population, scores)
    assert np.array_equal(np.load(tmp_path / "b" / "scores.npy"), scores[rows])


def test_dump_outputs_is_refused_for_other_workloads():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "bfgs",
                        "--dump-outputs", "unused"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "only the de workload" in r.stderr
