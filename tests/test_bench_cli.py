"""bench.py's command line: a plain run only times the steps, --full adds the other legs,
--dump-outputs writes what the last timed step computed (checked against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20251015          # bench.py's input seed
FULL_ONLY = ("roofline", "cpu_baseline", "cpu_reference_config0", "host_inclusive", "verified")


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                         capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    arrs = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert set(arrs) == {"groups", "parity", "recovered", "recovered_rows", "status"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    return arrs


def test_dump_outputs_samples_groups_within_the_budget(tmp_path):
    """More groups than fit: a seeded sample, the same on every call, under 64 MB."""
    import torch

    import bench
    G, m, bb, rmax = 120, 16, 9008, 16
    gen = torch.Generator().manual_seed(3)
    parity = torch.randint(0, 256, (G, m, bb), dtype=torch.uint8, generator=gen)
    out = torch.randint(0, 256, (G, rmax, bb), dtype=torch.uint8, generator=gen)
    rows = torch.randint(0, 128, (G, rmax), dtype=torch.uint8, generator=gen)
    status = torch.arange(G, dtype=torch.int32)
    n = bench.dump_outputs(str(tmp_path / "a"), SEED, 0, 1, parity, out, rows, status)
    assert 1 <= n < G
    a = _load(str(tmp_path / "a"))
    pick = a["groups"].astype(np.int64)
    assert len(pick) == n == len(set(pick)) and np.all(np.diff(pick) > 0) and pick[-1] < G
    assert np.array_equal(a["parity"], parity.numpy()[pick].astype(np.float32))
    assert np.array_equal(a["recovered"], out.numpy()[pick].astype(np.float32))
    assert np.array_equal(a["recovered_rows"], rows.numpy()[pick].astype(np.float32))
    assert np.array_equal(a["status"], pick.astype(np.float32))
    bench.dump_outputs(str(tmp_path / "b"), SEED, 0, 1, parity, out, rows, status)
    assert np.array_equal(_load(str(tmp_path / "b"))["groups"], a["groups"])
    # all groups when they fit
    assert bench.dump_outputs(str(tmp_path / "c"), SEED, 0, 1, parity[:9], out[:9], rows[:9],
                              status[:9]) == 9
    assert np.array_equal(_load(str(tmp_path / "c"))["groups"], np.arange(9))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path, oracle):
    from quic_amd import synth
    G, k, m, bb = 777, 10, 1, 1352
    d = str(tmp_path / "dump")
    line = _bench("--steps", "3", "--warmup", "1", "--groups", str(G), "--dump-outputs", d)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(G * k * 1350 / 2**30 / (line["ms_per_step"] * 1e-3),
                                          rel=5e-3)
    for key in FULL_ONLY:
        assert line[key] is None, key
    a = _load(d)
    assert np.array_equal(a["groups"], np.arange(G))
    data = synth.group_data(SEED, k, bb, G)
    exp, _ = oracle.encode_batch(k, m, bb, data)
    assert np.array_equal(a["parity"], exp.astype(np.float32))
    assert not a["status"].any()
    rows = a["recovered_rows"].astype(np.int64)           # one lost data row per group
    assert rows.shape == (G, 1) and rows.min() >= 0 and rows.max() < k
    assert np.array_equal(a["recovered"][:, 0], data[np.arange(G), rows[:, 0]].astype(np.float32))


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(tmp_path):
    line = _bench("--full", "--workload", "B", "--steps", "2", "--warmup", "1", "--groups", "257",
                  "--cpu-seconds", "0.2", "--host-steps", "1")
    assert line["full"] is True and line["steps"] == 2 and line["verified"] is True
    assert line["roofline"]["launch_ms"] > 0 and line["kernels"]["encode_ms"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["host_inclusive"]["status_ok"] is True
