"""bench.py's command line: a plain run measures the headline alone, --full turns
the side measurements on, --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _parse(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_has_no_side_measurement(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.steps == 7 and a.warmup == 3 and a.dump_outputs is None
    assert a.no_e2e and a.no_variants and a.no_sweeps and a.no_cpu_baseline and a.config4_frames == 0


def test_full_keeps_every_side_measurement_and_its_switch(monkeypatch):
    a = _parse(monkeypatch, ["--full"])
    assert a.full and not (a.no_e2e or a.no_variants or a.no_sweeps or a.no_cpu_baseline)
    assert a.config4_frames == 1_000_000
    a = _parse(monkeypatch, ["--full", "--no-sweeps", "--no-variants"])
    assert a.no_sweeps and a.no_variants and not a.no_e2e and a.config4_frames == 0


def test_config4_frames_without_full_is_refused(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, ["--config4-frames", "100"])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path, golden_vectors):
    """A plain 512-frame run: a short line with the headline keys and no side block, and
    DIR/*.npy holding the golden per-frame outcomes of config-2 frames 0..511 and their
    counters record."""
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--prewarm-ms", "0", "--frames", "512", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) <= 4096, p.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 3 and out["unit"] == "bit/s" and out["dtype"] == "f64"
    assert abs(out["value"] - 512 * 10240 / (out["ms_per_step"] / 1e3)) / out["value"] < 1e-9
    for k in ("roofline", "end_to_end", "variants", "config3_sweep", "config4", "cpu_baseline"):
        assert k not in out
    want_it = golden_vectors["c2_iters"][:512]
    want_sp = golden_vectors["c2_sp"][:512].astype(bool)
    got = {n: np.load(out_dir / (n + ".npy")) for n in out["dumped_outputs"]}
    assert sorted(got) == ["counters", "iterations", "keys_match", "syndromes_match"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert (got["iterations"] == want_it).all() and (got["syndromes_match"] == want_sp).all()
    assert (got["keys_match"][want_sp] == 1).all()          # (config 2: every frame decodes to Alice's key)
    it = want_it[want_sp].astype(np.int64)
    assert got["counters"].tolist() == [512, int(want_sp.sum()), int(want_sp.sum()), int(it.sum()),
                                        int((it * it).sum()), int(it.min()), int(it.max())]
