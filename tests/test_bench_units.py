"""bench.py's pure-Python pieces on the CPU: the byte model behind `roofline.frac`, the HBM plan that decides
whether a run is refused up front (item 1), which sources of a rank run in series, and what --dump-outputs writes."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Solver:
    def kernel_name(self, ps):
        return "k_test (a test kernel)"


def _roof(ps, S, as_group):
    a = types.SimpleNamespace(config=None, bin=None, batch_edges=None, no_ceilings=True)
    eng = types.SimpleNamespace(build_id=lambda: "0123456789abcdef")
    base = dict(persist_launches=0, binned_sweeps=0, sweep_launches=0, iterations=10, push_launches=10, push_ms=1.0, sum_F=1000, sum_E=100000, sum_N=1000)
    return bench.roofline_block(a, dict(base, **ps), S, as_group, _Solver(), eng, 0, 5)


def test_sweeps_are_priced_at_what_they_must_move_and_pushes_at_surveys_unit():
    F, E, N, t = 1000, 100000, 1000, 1e-3
    push = _roof({}, 1, False)
    assert push["form"] == "push" and abs(push["achieved"] - (72 * F + 24 * E + 4 * N) / t / 1e9) < 1e-2
    assert abs(push["work_rate_survey_unit"]["GBps"] - push["achieved"]) < 1e-2 and "24 E" in push["bytes_model"]
    for form, ps in (("pull", dict(sweep_launches=10)), ("binned", dict(sweep_launches=10, binned_sweeps=10)), ("resident", dict(persist_launches=10))):
        r = _roof(ps, 1, False)
        assert r["form"] == form and abs(r["achieved"] - (72 * F + 12 * E + 4 * N) / t / 1e9) < 1e-2     # one source: 8 + 4 bytes per active edge
        assert r["work_rate_survey_unit"]["GBps"] > r["achieved"] and "(8 + 4 / 1)" in r["bytes_model"]
        assert abs(r["frac"] - r["achieved"] / 8000.0) < 1e-5 and r["frac_traffic"] is None and r["traffic"] is None
    g = _roof(dict(sweep_launches=10), 10, True)                                                          # ten sources share the column entry
    assert abs(g["achieved"] - (72 * F + 8.4 * E + 4 * N) / t / 1e9) < 1e-2 and "(8 + 4 / 10)" in g["bytes_model"]
    s = _roof(dict(sweep_launches=10, binned_sweeps=10), 3, False)                                        # three sources IN SERIES: single-source pricing
    assert "(8 + 4 / 1)" in s["bytes_model"]


def test_hbm_plan_counts_what_the_engine_holds():
    V, W, c = 1 << 25, 146_836_518, 1_468_365
    ring = bench.hbm_plan(V, W, 1, c, 1, False, True, bench.RING)
    pre = bench.hbm_plan(V, W, 1, c, 1, False, True, 26)
    assert ring["resident_epochs"] == 3 and pre["plan_bytes"] - ring["plan_bytes"] == 23 * ring["epoch_bytes"]
    assert 2.5e9 < ring["epoch_bytes"] < 5e9 and 15e9 < ring["plan_bytes"] < 40e9       # (measured on the twitter stand-in: 24.5 GB peak)
    und = bench.hbm_plan(V, W, 0, c, 1, False, True, 3)
    assert und["epoch_bytes"] > 1.8 * ring["epoch_bytes"]                                # an undirected window holds both orientations
    g10 = bench.hbm_plan(1 << 27, 180_606_713, 0, 100_000, 10, True, False, 3)
    assert g10["source_state_bytes"] == 416 * (1 << 27) and 80e9 < g10["plan_bytes"] < 110e9   # friendster group: 89.6 GB measured
    assert 26 * g10["epoch_bytes"] + g10["engine_bytes"] + g10["source_state_bytes"] > 0.75 * 288e9   # what pre-staging the driver's step counts would have asked for


def test_series_policy_constants():
    assert bench.SERIES_MAX == 3 and bench.BIG_WINDOW == 4_000_000 and bench.RING == 3 and bench.CPU_SAMPLE_BATCHES == 6


class _States:
    """p / r of n sources over V vertices, as solver.read(i) hands them out."""

    def __init__(self, n, V):
        rng = np.random.default_rng(7)
        self.p = [rng.random(V) for _ in range(n)]
        self.r = [rng.random(V) * 1e-10 - 5e-11 for _ in range(n)]

    def read(self, i):
        return self.p[i].copy(), self.r[i].copy()


def test_dump_outputs_whole_arrays_when_they_fit(tmp_path):
    s = _States(3, 1000)
    bench.dump_outputs(str(tmp_path), s, 3, 1000, 0, 1)
    z = {f.name[:-4]: np.load(f) for f in tmp_path.iterdir()}
    assert set(z) == {"vertices", "p", "r", "p_sum", "r_max_abs"} and all(a.dtype == np.float64 for a in z.values())
    assert np.array_equal(z["vertices"], np.arange(1000)) and np.array_equal(z["p"], np.stack(s.p)) and np.array_equal(z["r"], np.stack(s.r))
    assert np.array_equal(z["p_sum"], [np.sum(p) for p in s.p]) and np.array_equal(z["r_max_abs"], [np.max(np.abs(r)) for r in s.r])


def test_dump_outputs_fixed_sample_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 20) + 72_000)   # room for 1 000 vertices: p and r of 4 sources + the id (72 bytes each) + 1 MB
    s = _States(4, 5000)
    bench.dump_outputs(str(tmp_path / "a"), s, 4, 5000, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), s, 4, 5000, 0, 1)
    a = {f.name[:-4]: np.load(f) for f in (tmp_path / "a").iterdir()}
    b = {f.name[:-4]: np.load(f) for f in (tmp_path / "b").iterdir()}
    ids = a["vertices"].astype(np.int64)
    assert len(ids) == 1000 and np.all(np.diff(ids) > 0) and ids[-1] < 5000           # a sorted sample without repeats
    assert all(np.array_equal(a[k], b[k]) for k in a)                                  # ... the same one every time
    assert np.array_equal(a["p"], np.stack(s.p)[:, ids]) and np.array_equal(a["r"], np.stack(s.r)[:, ids])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_BYTES
    bench.dump_outputs(str(tmp_path / "c"), s, 4, 5000, 1, 2)                           # N > 1: per rank, the budget shared
    assert len(np.load(tmp_path / "c" / "rank1_vertices.npy")) == 500


def test_cpu_leg_beyond_its_budget_is_a_bounded_sample(tmp_path, monkeypatch):
    """A long run (--steps in the hundreds) cannot wait for the live CPU leg to follow every batch: past CPU_FOLLOW_BUDGET_S
    (projected) it stops as a bounded sample, compares nothing and says why; within the budget it compares at the end."""
    from dynamicppr_amd import datagen, stream as st
    V, e1, e2, cfg = datagen.stand_in_stream("dblp", str(tmp_path))
    f = cfg.flags.split()
    opt = {f[i]: f[i + 1] for i in range(0, len(f), 2)}
    wl = st.workload_config(cfg.edges, 0.1, 0, float(opt["-r"]), int(opt["-b"]), 0, 0)
    src = [int(s) for s in datagen.top_sources(V, e1, e2, wl.window, cfg.directed, 1)]
    p_end = [np.zeros(V)]
    monkeypatch.setattr(bench, "CPU_FOLLOW_BUDGET_S", 0.0)
    cut = bench.cpu_baseline(V, e1, e2, cfg.directed, wl.window, wl.per_batch, src, 1e-9, 40, p_end, cfg.edges)
    assert cut["max_abs_dp"] is None and cut["p_cpu"] is None and "projected" in cut["bounded"]
    assert f"{bench.CPU_SAMPLE_BATCHES} batches of the same stream" in cut["sample"] and cut["t1_value"] > 0
    monkeypatch.setattr(bench, "CPU_FOLLOW_BUDGET_S", 1e9)
    full = bench.cpu_baseline(V, e1, e2, cfg.directed, wl.window, wl.per_batch, src, 1e-9, 8, p_end, cfg.edges)
    assert "bounded" not in full and full["max_abs_dp"] > 0 and len(full["p_cpu"]) == 1
