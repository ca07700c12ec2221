"""`yacht run --gather --gather_top K` over a cohort, on the GPU: the block's ranking on the device (yh_explain_members_rows_device
+ one yh_gather_batch_device per gather coverage in cohort._Device) against what it must equal.

From files: every results/<stem>/gather_profile.tsv of the fixture cohort of tests/test_gpu_cohort.py equals, byte for byte, the
file a single-sample run of that sample writes with the same options, and results/cohort_gather.tsv holds the same rows in long
form; the cohort by default and under YACHT_COHORT_GATHER=loop, each in a fresh child process, leave the same results/ tree
(archives compared as tests/test_gpu_cohort_residual_device.py compares them).  A cohort with duplicate organism names takes
the host form for the recomputed sample only.  At the level of cohort._Device: the rows collect() returns equal RefDB.gather on
call sets read from the same block's present rows -- also with a capacity so small that the block takes the dense fallback."""
import json
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pandas as pd
import pytest
from test_gpu_cohort import trained as fixture_cohort  # noqa: F401  (the module's fixture, made again for this module)
from test_gpu_cohort_residual_device import _same_tree, _synthetic
from test_gpu_residual_e2e import A, B, _run, trained  # noqa: F401

from yacht_amd import cohort, gather
from yacht_amd.engine import RefDB
from yacht_amd.hypothesis_recovery_src import hyp_test_native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = ["--gather", "--gather_top", "50"]


def _children(cfg, files, outdirs, opts):
    """The cohort command in fresh child processes, side by side: outdirs = {directory: YACHT_COHORT_GATHER or None}."""
    running = []
    for outdir, mode in outdirs.items():
        outdir.mkdir()
        env = {k: v for k, v in os.environ.items() if k != "YACHT_COHORT_GATHER"}
        if mode is not None:
            env["YACHT_COHORT_GATHER"] = mode
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        running.append(subprocess.Popen([sys.executable, "-m", "yacht_amd", "run", "--json", str(cfg), "--sample_file", *map(str, files),
                                         "--num_threads", "2", "--outdir", str(outdir), *opts], env=env, cwd=ROOT,
                                        stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    for child in running:
        _out, err = child.communicate()
        assert child.returncode == 0, err[-2000:]
    return [outdir / "results" for outdir in outdirs]


def _long_form_equals_the_files(res, stems):
    """cohort_gather.tsv = the samples' gather_profile.tsv files one after the other, behind a sample column."""
    want = ["\t".join(["sample"] + gather.GATHER_COLUMNS)]
    for stem in stems:
        path = res / stem / gather.GATHER_NAME
        if path.exists():
            want += [f"{stem}\t{line}" for line in path.read_text().splitlines()[1:]]
    assert (res / gather.COHORT_GATHER_NAME).read_text().splitlines() == want
    return len(want) - 1


def _equals_single_runs(res, cfg, files, tmp_path, opts):
    stems = [cohort.sample_stem(str(f)) for f in files]
    n_ranked = 0
    for f, stem in zip(files[:4], stems):
        single = _run(cfg, [f], tmp_path / f"single_{stem}", *opts)
        assert (res / stem / gather.GATHER_NAME).read_bytes() == (single / gather.GATHER_NAME).read_bytes(), stem
        n_ranked += len(pd.read_csv(single / gather.GATHER_NAME, sep="\t"))
    assert not (res / "none").exists()  # no overlap: no folder, no ranking
    assert _long_form_equals_the_files(res, stems) == n_ranked > 0


def test_fixture_cohort_equals_single_runs(hip_lib, fixture_cohort, tmp_path):  # noqa: F811
    tmp, cfg, files = fixture_cohort
    opts = TOP + ["--min_coverage_list", "1", "0.05", "0.001"]
    _equals_single_runs(_run(cfg, files, tmp_path / "cohort", *opts), cfg, files, tmp_path, opts)


def test_fixture_cohort_with_abundance_and_residual_and_the_loop(hip_lib, fixture_cohort, tmp_path):  # noqa: F811
    """The default and the YACHT_COHORT_GATHER=loop run, each a fresh child process, leave the same tree, and its rankings are
    the single runs'."""
    tmp, cfg, files = fixture_cohort
    opts = TOP + ["--min_coverage_list", "1", "0.05", "0.001", "--abundance", "--residual"]
    res, looped = _children(cfg, files, {tmp_path / "device": None, tmp_path / "loop": "loop"}, opts)
    names = _same_tree(str(res), str(looped), "device against loop")
    assert gather.COHORT_GATHER_NAME in names and all(f"{cohort.sample_stem(str(f))}/{gather.GATHER_NAME}" in names for f in files[:4])
    _equals_single_runs(res, cfg, files, tmp_path, opts)


def test_the_cap_and_the_other_options_reach_the_block(hip_lib, trained, tmp_path):  # noqa: F811
    """--gather_top 1, --gather_min_hits and --gather_coverage on a cohort whose samples have two organisms to rank: byte for
    byte the single runs, cut at one row."""
    tmp, cfg3, cfg4, sketch, files = trained
    paths = [files["mix"], files["second"], files["none"], files["mix_flat"]]
    full = _run(cfg4, paths, tmp_path / "full", "--gather", "--gather_top", "50", "--min_coverage_list", "1", "0.5", "0.1")
    assert len(pd.read_csv(full / "mix" / gather.GATHER_NAME, sep="\t")) >= 6  # at least two organisms at each coverage
    opts = ["--gather", "--gather_top", "1", "--gather_min_hits", "5", "--gather_coverage", "0.1", "1", "--min_coverage_list", "1", "0.5", "0.1"]
    res = _run(cfg4, paths, tmp_path / "cohort", *opts)
    for name in ("mix", "second", "mix_flat"):
        single = _run(cfg4, [files[name]], tmp_path / f"single_{name}", *opts)
        assert (res / name / gather.GATHER_NAME).read_bytes() == (single / gather.GATHER_NAME).read_bytes(), name
        got = pd.read_csv(res / name / gather.GATHER_NAME, sep="\t")
        assert got["min_coverage"].tolist() == [1.0, 0.1] and got["rank"].tolist() == [0, 0]
    assert _long_form_equals_the_files(res, ["mix", "second", "none", "mix_flat"]) == 6
    flat = pd.read_csv(res / "mix_flat" / gather.GATHER_NAME, sep="\t")
    assert (flat["abund_sum_unique"] == flat["num_unique"]).all()  # a sketch without abundances counts every hash once


def test_duplicate_names_take_the_host_form_for_the_recomputed_sample_only(hip_lib, trained, tmp_path, monkeypatch):  # noqa: F811
    """A takes B's organism name: the sample of B pulls A's row in by name, its tables are recomputed on the host and its
    ranking takes the host-form calls; the other sample's comes from the block's pass."""
    tmp, cfg3, cfg4, sketch, files = trained
    conf = json.load(open(cfg4))
    man = pd.read_csv(conf["manifest_file_path"], sep="\t")
    man.loc[man["organism_name"] == A, "organism_name"] = B
    dup_man = tmp_path / "dup_manifest.tsv"
    man.to_csv(dup_man, sep="\t", index=False)
    conf["manifest_file_path"] = str(dup_man)
    dup_cfg = tmp_path / "dup_config.json"
    dup_cfg.write_text(json.dumps(conf))
    opts = TOP + ["--min_coverage_list", "1", "0.2", "--show_all"]
    paths = [files["b_twice"], files["mix"]]
    calls, res = {}, {}
    real = gather.gather_call_sets
    for mode in ("device", "loop"):
        count = []
        monkeypatch.setattr(gather, "gather_call_sets", lambda *a, _c=count, **k: (_c.append(1), real(*a, **k))[1])
        if mode == "loop":
            monkeypatch.setenv("YACHT_COHORT_GATHER", "loop")
        else:
            monkeypatch.delenv("YACHT_COHORT_GATHER", raising=False)
        res[mode] = _run(dup_cfg, paths, tmp_path / mode, *opts)
        calls[mode] = len(count)
    monkeypatch.delenv("YACHT_COHORT_GATHER", raising=False)
    monkeypatch.setattr(gather, "gather_call_sets", real)
    _same_tree(str(res["device"]), str(res["loop"]), "duplicate names")
    summary = pd.read_csv(res["device"] / "cohort_samples.tsv", sep="\t").set_index("stem")
    recomputed = []
    for stem in ("b_twice", "mix"):
        df = pd.read_csv(res["device"] / stem / "result_all.txt", sep="\t")
        if int((df["min_coverage"] == 1.0).sum()) != int(summary.loc[stem, "n_overlapping"]):
            recomputed.append(stem)
    assert "b_twice" in recomputed and calls == {"device": len(recomputed), "loop": 2}
    for f, stem in zip(paths, ("b_twice", "mix")):
        single = _run(dup_cfg, [f], tmp_path / f"single_{stem}", *opts)
        assert (res["device"] / stem / gather.GATHER_NAME).read_bytes() == (single / gather.GATHER_NAME).read_bytes(), stem


# ---- cohort._Device ----------------------------------------------------------------------------------------------------------
def _check_block_gather(db, block, abunds, got, covs, n_user, gather_sets, min_hits, top, what):
    """rows / counts of collect() against RefDB.gather on the call sets of the block's own present rows."""
    rows, _pv, pres, _ncov = got[:4]
    g_rows, g_n = got[-1]
    first = len(covs) - n_user
    assert g_rows.shape[:2] == (len(gather_sets), len(block)) == g_n.shape and g_rows.dtype == cohort_row_dtype()
    n_ranked = 0
    for s, sample in enumerate(block):
        sel = rows[:, 0] == s
        for g, u in enumerate(gather_sets):
            call_set = rows[sel, 1][pres[first + u, sel] != 0].astype(np.int64)
            want = db.gather(sample, gather.candidate_table(db.n_refs, call_set), None if abunds is None else abunds[s],
                             min_hits=min_hits, cap_rows=top)[0]
            assert int(g_n[g, s]) == len(want) and np.array_equal(g_rows[g, s, :len(want)], want), (what, s, g)
            n_ranked += len(want)
    return n_ranked


def cohort_row_dtype():
    from yacht_amd.engine import GATHER_ROW_DTYPE
    return GATHER_ROW_DTYPE


NINE = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1]


@pytest.mark.parametrize("covs,n_user,gather_sets,with_residual", [([1.0, 0.5, 0.05], 3, [0, 2], False), ([1.0] + NINE, 9, [1, 6, 7, 8], True)])
def test_device_blocks_against_the_single_call(hip_lib, covs, n_user, gather_sets, with_residual):
    """Two blocks back to back on one _Device, the second smaller (65 samples, then 20); abundances for two samples in three;
    gather coverages in both passes of seven call sets; with and without the explain pass beside it."""
    values, offsets, samples, abunds = _synthetic(85)
    with RefDB(values, offsets) as db:
        n_max = int(np.max(db.sizes))
        tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        dev = cohort._Device(db, covs, 31, 0.95, tab[5], residual_sets=n_user if with_residual else 0, gather_sets=gather_sets,
                             gather_min_hits=2, gather_top=3, n_user=n_user, max_samples=65)
        timer = defaultdict(float)
        for lo, hi in ((0, 65), (65, 85)):
            got = dev.collect(dev.launch(samples[lo:hi], None, abunds[lo:hi]), timer)
            assert len(got) == (6 if with_residual else 5)
            assert _check_block_gather(db, samples[lo:hi], abunds[lo:hi], got, covs, n_user, gather_sets, 2, 3, f"block {lo}") > 20
            assert int(got[-1][1].max()) == 3  # some ranking is cut at the cap
        assert timer["dense_fallback_blocks"] == 0 and timer["gpu_gather"] > 0
        got = dev.collect(dev.launch(samples[:9]), timer)  # without abundances every hash counts once
        _check_block_gather(db, samples[:9], None, got, covs, n_user, gather_sets, 2, 3, "no abundances")
        assert all(np.array_equal(got[-1][0][g, s, :k]["w_unique"], got[-1][0][g, s, :k]["n_unique"])
                   for g in range(len(gather_sets)) for s, k in enumerate(got[-1][1][g]))


def test_device_dense_fallback_reruns_the_ranking(hip_lib):
    values, offsets, samples, abunds = _synthetic(50)
    covs = [1.0, 0.1]
    with RefDB(values, offsets) as db:
        n_max = int(np.max(db.sizes))
        tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        dev = cohort._Device(db, covs, 31, 0.95, tab[5], cap=64, gather_sets=[0, 1], gather_top=50, n_user=2, max_samples=30)
        timer = defaultdict(float)
        first = dev.collect(dev.launch(samples[:30], None, abunds[:30]), timer)
        assert first[0].shape[0] > 64 and timer["dense_fallback_blocks"] == 1 and dev.cap > first[0].shape[0]
        assert _check_block_gather(db, samples[:30], abunds[:30], first, covs, 2, [0, 1], 1, 50, "dense") > 20
        second = dev.collect(dev.launch(samples[30:50], None, abunds[30:50]), timer)
        assert timer["dense_fallback_blocks"] == 1
        assert _check_block_gather(db, samples[30:50], abunds[30:50], second, covs, 2, [0, 1], 1, 50, "compact after growth") > 10
