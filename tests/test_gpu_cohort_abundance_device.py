"""`yacht run --abundance` over a cohort with the block's depth pass on the device in one call (yh_abund_batch_device in
cohort._Device.abundance_pass) against the per-sample loop of yh_abund_device it replaces (YACHT_COHORT_ABUND=loop).

The fixture cohort of test_gpu_cohort.py, with --abundance and with --abundance --residual, each run by default and under
YACHT_COHORT_ABUND=loop, each in a fresh child process: the two settings must leave the same results/ tree.  Plain files
are compared byte for byte.  A zip archive (result.xlsx, residual.sig.zip) stamps every entry with the time it was written,
so two runs never give the same archive bytes: those are compared by what they hold, as test_gpu_cohort_residual_device.py
does (entry by entry, byte for byte; the residual sketch by its loaded signature)."""
import os
import subprocess
import sys

import pandas as pd
import pytest
from test_gpu_cohort import trained  # noqa: F401  (the module's fixture, made again for this module)
from test_gpu_cohort_residual_device import _same_tree

from yacht_amd import cohort

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "import sys\nsys.path.insert(0, sys.argv[1])\nfrom yacht_amd import cli\nsys.exit(cli.main(sys.argv[2:]))\n"


def _cohort_in_a_child(cfg, files, outdir, opts, loop):
    env = {k: v for k, v in os.environ.items() if k != "YACHT_COHORT_ABUND"}
    if loop:
        env["YACHT_COHORT_ABUND"] = "loop"
    outdir.mkdir()
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, "run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2",
                        "--outdir", str(outdir), *opts], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return outdir / "results"


@pytest.mark.parametrize("opts", [["--abundance"], ["--abundance", "--residual"]], ids=["abundance", "abundance+residual"])
def test_the_batched_pass_writes_the_files_of_the_per_sample_loop(hip_lib, trained, tmp_path, opts):  # noqa: F811
    _tmp, cfg, files = trained
    batched = _cohort_in_a_child(cfg, files, tmp_path / "batched", opts, loop=False)
    looped = _cohort_in_a_child(cfg, files, tmp_path / "looped", opts, loop=True)
    names = _same_tree(str(batched), str(looped), " ".join(opts))
    assert "cohort_presence.tsv" in names and "cohort_samples.tsv" in names
    pres = pd.read_csv(batched / "cohort_presence.tsv", sep="\t")
    assert list(pres.columns)[-len(cohort.PRESENCE_ABUNDANCE_COLUMNS):] == cohort.PRESENCE_ABUNDANCE_COLUMNS
    full = pd.read_csv(batched / "full" / "result_all.txt", sep="\t")  # (the depth columns hold values: not a comparison of blanks)
    assert "abund_median_exclusive" in full.columns and bool((full["abund_sum_overlap"] > 0).any())
