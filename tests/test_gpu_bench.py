"""bench.py's JSON line on the GPU (one rank, small batches): the fields the
round-end bench and the judge read -- the HIP-event roofline of the dominant
kernel, the memory-only pattern floor of the transforms (roofline.pattern_floor_ms,
timed after the timed region from the tools library), per-kernel medians,
transforms/s for fwd+inv, and the oracle check of the sampled polynomials."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=240):
    env = {**os.environ, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_headline_line_carries_pattern_floor(ntt):
    d = _bench(["--config", "3", "--batch", "8192", "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline"])
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert set(r["per_kernel_ms"]) == {"fwd", "inv"} and set(r["per_kernel_median_ms"]) == {"fwd", "inv"}
    floor = r["pattern_floor"]
    assert set(floor["ms"]) == {"fwd", "inv"} and all(v > 0 for v in floor["ms"].values())
    assert r["pattern_floor_ms"] == floor["ms"][r["kernel"]]
    assert abs(r["kernel_over_floor"] - r["avg_launch_ms"] / r["pattern_floor_ms"]) < 1e-9
    assert 0.3 < r["kernel_over_floor"] < 5.0
    assert d["transforms_per_s"] == pytest.approx(2 * d["value"])
    assert d["check"]["roundtrip_identity_full_batch"] is True
    s = d["check"]["sampled_vs_oracle"]
    assert s["ok"] is True and s["polys"] == 4096   # ~4096 sampled + first/last (np.unique may merge a few)


@pytest.mark.parametrize("config", [3, 4])
def test_plain_run_is_lean_and_dumps_last_step(ntt, oracle, tmp_path, config):
    """Without --full the line carries the timed region's own figures only (no
    checker leg, CPU baseline, pattern floor or latency leg); --dump-outputs
    writes a fixed sample of the last step's output rows as float64, here
    checked against the oracle on the regenerated inputs."""
    import numpy as np
    import bench
    batch, steps = 4099, 3   # odd, above the 1024 rows a dumped n = 2048 array holds
    d = _bench(["--gpus", "1", "--config", str(config), "--batch", str(batch), "--steps", str(steps), "--warmup", "1",
                "--dump-outputs", str(tmp_path)])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["value"] == pytest.approx(batch * steps / (d["ms_per_step"] * steps * 1e-3))
    assert d["cpu_baseline"] is None and "cpu_baseline_parallel" not in d
    assert d["check"] == {"roundtrip_identity_full_batch": None, "sampled_vs_oracle": None}
    hbm = d["roofline"] if config == 3 else d["roofline"]["hbm"]
    assert "pattern_floor" not in hbm and "latency" not in d["roofline"] and hbm["avg_launch_ms"] > 0
    names = {"rows", "x", "x_fwd"} if config == 3 else {"rows", "z"}
    assert set(d["dumped_outputs"]) == names == {f[:-4] for f in os.listdir(tmp_path)}
    got = {k: np.load(tmp_path / f"{k}.npy") for k in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    rows = got["rows"].astype(np.int64)
    assert np.array_equal(rows, bench.dump_rows(batch, 2048)) and len(rows) == 1024
    assert rows[0] == 0 and rows[-1] == batch - 1 and np.all(np.diff(rows) > 0)
    a = np.concatenate([oracle.fill_uniform(1, "p-III", bench.SEED, int(r)) for r in rows])
    if config == 3:
        assert np.array_equal(got["x"], a) and np.array_equal(got["x_fwd"], oracle.poly_ntt(a, "p-III"))
    else:
        b = np.concatenate([oracle.fill_uniform(1, "p-III", bench.SEED ^ 0xFFFF, int(r)) for r in rows])
        assert np.array_equal(got["z"], oracle.poly_mul(a, b, "p-III"))


@pytest.mark.parametrize("config", [4, 5])
def test_valu_bound_lines_have_no_floor(ntt, config):
    """Products are VALU-bound: their roofline is the VALU one, with no
    transform pattern floor."""
    d = _bench(["--config", str(config), "--batch", "2048", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert d["roofline"]["bound"] == "valu" and "pattern_floor" not in d["roofline"]["hbm"]
    assert d["transforms_per_s"] is None and d["check"]["sampled_vs_oracle"]["ok"] is True
