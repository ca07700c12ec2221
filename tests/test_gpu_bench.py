"""GPU: bench.py's plain run -- exactly --steps timed steps, `ms_per_step` on the line, and --dump-outputs: the counts of the
last timed step, the same from run to run and equal to the CPU oracle on the same synthetic database and sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("overlap", "n_exclusive", "n_matches")
REFS, SAMPLE_HASHES, SAMPLES, PRESENT, SEED, STEPS, WARMUP = 4000, 100_000, 3, 50, 1002, 7, 2


def _plain_run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--refs", str(REFS), "--sample-hashes", str(SAMPLE_HASHES), "--samples", str(SAMPLES),
                        "--present", str(PRESENT), "--seed", str(SEED), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_steps_and_dumped_outputs(hip_lib, tmp_path):
    line = _plain_run(tmp_path / "a")
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["metric"].startswith("ref-sketch containment queries/sec") and line["unit"] == "queries/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] - REFS / (line["ms_per_step"] / 1e3)) / line["value"] < 0.05  # (ms_per_step is rounded to 0.1 us)
    assert line["cpu_baseline"] is None and line["roofline"] is None and "extras" not in line  # (those are --full)
    _plain_run(tmp_path / "b")
    got = {}
    for n in NAMES:
        a = np.load(tmp_path / "a" / f"{n}.npy")
        assert a.dtype == np.float64 and a.shape == (REFS,)
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{n}.npy")), n
        got[n] = a
    assert got["overlap"].sum() > 0

    # the last timed step took sample (WARMUP + STEPS - 1) mod SAMPLES of bench.py's workload: the oracle on the same arrays
    from oracle import oracle
    from yacht_amd import synth

    plan = synth.global_db_plan(SEED, REFS, cluster_frac=0.10, median=3300.0, sigma=0.6, lo=300, hi=15000)
    values, offsets = synth.global_db_refs_device(plan, np.arange(REFS), device="cuda:0")
    i = (WARMUP + STEPS - 1) % SAMPLES
    sample = synth.global_db_sample_device(plan, SEED + 1000 + i, n_sample=SAMPLE_HASHES, n_present=PRESENT, device="cuda:0")
    hv, ho, hs = (t.cpu().numpy().view(np.uint64) for t in (values, offsets, sample))
    want_ov = oracle.overlap(hv, ho, hs, threads=4)
    want_e, want_m = oracle.exclusive(hv, ho, want_ov > 0, hs)
    for n, want in zip(NAMES, (want_ov, want_e, want_m)):
        assert np.array_equal(got[n], want.astype(np.float64)), n
