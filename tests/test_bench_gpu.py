"""bench.py's output contract on the GPU, at a small batch: one JSON line with the BASELINE metric, a whole-job value
consistent with its own step time; with --full the roofline object of the dominant kernel and every block's DAH checked
against the committed digests (the timed steps' output, tests/golden/bench_digests.json); a plain run's line without
them, and the outputs --dump-outputs writes."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_and_dump(tmp_path):
    """A plain run prints the headline alone (nothing of --full), and --dump-outputs writes the last timed step's
    outputs: every DAH equals the committed digest of its seed, the sampled EDS cells of the original quadrant are
    the input shares, and the files are float32 / float64 within the size limit."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    k, B, w = 128, 8, 256
    out = tmp_path / "dump"
    d = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--dump-outputs", str(out))
    assert d["metric"] == bench.METRIC and d["unit"] == "blocks/s" and d["dtype"] == "u8"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(B * 1000.0 / d["ms_per_step"], rel=1e-3)
    for key in ("roofline", "kernel_rooflines", "hbm_ceilings", "output_check", "kernels_ms", "k512_split",
                "c2_single_block", "cpu_baseline"):
        assert key not in d, key
    files = {f: np.load(out / f) for f in os.listdir(out)}
    assert set(files) == {"dah.npy", "status.npy", "roots.npy", "roots_block_index.npy", "eds_cells.npy",
                          "eds_cell_index.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 1000 * 1000
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_digests.json")))[f"k{k}"]
    dah = files["dah.npy"].astype(np.uint8)
    assert [bytes(r).hex() for r in dah] == [want[str(0xC0FFEE + b)] for b in range(B)]
    assert np.array_equal(files["status.npy"], np.full(B, -1.0))
    assert files["roots.npy"].shape == (B, 2 * w, 90)
    assert np.array_equal(files["roots_block_index.npy"], np.arange(B))
    idx = files["eds_cell_index.npy"].astype(np.int64)
    cells = files["eds_cells.npy"]
    assert cells.shape == (len(idx), 512) and np.all(np.diff(idx) > 0) and idx[-1] < B * w * w
    ods = np.stack([bench.gen_ods(k, 0xC0FFEE + b) for b in range(B)]).reshape(B, k, k, 512)
    b, r, c = idx // (w * w), idx // w % w, idx % w
    q0 = (r < k) & (c < k)
    assert q0.sum() > 1000
    assert np.array_equal(cells[q0], ods[b[q0], r[q0], c[q0]].astype(np.float32))


def test_bench_line_contract():
    d = _bench("--steps", "3", "--warmup", "1", "--batch", "8", "--full", "--no-extras", "--no-cpu-baseline",
               "--no-k512-split")
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"]
    for key in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    # value = blocks of all ranks / elapsed, ms_per_step = elapsed / steps
    assert d["value"] == pytest.approx(8 * 1000.0 / d["ms_per_step"], rel=1e-3)
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["peak"] > 0 and 0 < r["frac"] <= 1 and r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-2)
    assert d["output_check"]["blocks_checked_vs_golden"] == 8
