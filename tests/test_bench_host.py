"""bench.py's host-side pieces on the CPU: the device count taken without HIP (the parent of `--gpus N` must not
initialise the GPU before it starts the ranks), and the like-for-like CPU baseline (burn-in window untimed, the
GPU's timed window timed inside the oracle, mcmc.c:140-185)."""
import os

import bench

HERE = os.path.dirname(os.path.abspath(__file__))


def _node(root, name, simds):
    d = root / name
    d.mkdir()
    (d / "properties").write_text("cpu_cores_count 0\nsimd_count %d\nmem_banks_count 1\n" % simds)


def test_visible_gpu_count_from_kfd_topology(tmp_path, monkeypatch):
    for v in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    _node(tmp_path, "0", 0)        # the CPU agent
    for k in range(1, 9):
        _node(tmp_path, str(k), 1024)
    assert bench.visible_gpu_count(str(tmp_path)) == 8
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "2,5")
    assert bench.visible_gpu_count(str(tmp_path)) == 2
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "3")
    assert bench.visible_gpu_count(str(tmp_path)) == 1
    assert bench.visible_gpu_count(str(tmp_path / "missing")) is None


def test_dump_outputs_files_dtypes_and_budget(tmp_path, monkeypatch):
    import numpy as np
    rng = np.random.default_rng(1)
    k, T, W, C = 3, 40, 11, 5
    gathered = rng.random((C, 4))
    sel_ab = rng.integers(0, 300, (k, T, W)).astype(np.int16)
    sel_cdl, chain_cdl = rng.random((k, T, 3)), rng.random((C, T, 3))
    d = tmp_path / "dump"
    bench.dump_outputs(str(d), gathered, [4, 0, 2], sel_ab, sel_cdl, chain_cdl)
    got = {p.name[:-4]: np.load(p) for p in d.iterdir()}
    assert sorted(got) == ["chain_cdl", "chain_cdl_calls", "selected_chains", "selected_records_ab_pi",
                           "selected_records_calls", "selected_records_cdl", "summaries"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["selected_records_ab_pi"], sel_ab) and np.array_equal(got["chain_cdl"], chain_cdl)
    assert np.array_equal(got["selected_records_calls"], np.arange(T)) and got["selected_chains"].tolist() == [4, 0, 2]
    # over the budget: the same sorted sample of the saved calls every time, and the arrays fit
    monkeypatch.setitem(bench.DUMP_BUDGET, "selected_records_ab_pi", k * W * 4 * 7)
    for name in ("d1", "d2"):
        bench.dump_outputs(str(tmp_path / name), gathered, [4, 0, 2], sel_ab, sel_cdl, chain_cdl)
    a, b = (np.load(tmp_path / n / "selected_records_calls.npy").astype(int) for n in ("d1", "d2"))
    assert np.array_equal(a, b) and len(a) == 7 and (np.diff(a) > 0).all() and a.max() < T
    assert np.array_equal(np.load(tmp_path / "d1" / "selected_records_ab_pi.npy"), sel_ab[:, a])
    assert np.array_equal(np.load(tmp_path / "d1" / "selected_records_cdl.npy"), sel_cdl[:, a])
    assert (tmp_path / "d1" / "selected_records_ab_pi.npy").stat().st_size <= k * W * 4 * 7 + 256


def test_cpu_baseline_times_the_window_after_burnin():
    ds = os.path.join(HERE, "golden", "datasets", "g5s5.txt")
    r = bench.cpu_baseline(ds, 4, 6, 2)
    assert r["value"] > 0 and r["cores"] == 2 and r["kind"] == "port"
    assert "4 untimed" in r["sample"] and "6 timed" in r["sample"]
    assert r["from_birth"]["value"] > 0
    r0 = bench.cpu_baseline(ds, 0, 3, 1)
    assert "from_birth" not in r0
