"""`yacht run --residual` over a cohort with the block's residual on the device (yh_explain_members_rows_device +
yh_explain_batch_device in cohort._Device) against the per-sample host-form path it replaces.

From files: the same cohort run twice, by default and under YACHT_COHORT_EXPLAIN=host, must leave the same results/ tree.
Plain files are compared byte for byte.  The two kinds of zip archive are compared by what they hold, because a zip entry
carries the time it was written: result.xlsx entry by entry, residual.sig.zip by its loaded signatures (as
test_gpu_residual_e2e.py compares a cohort with a single run).  At the level of cohort._Device: for every sample of a block
the flags and totals that collect() returns equal residual.explain_call_sets on call sets read from the same block's
present rows -- with a capacity so small that the block takes the dense fallback, and over two blocks back to back, the
second smaller."""
import json
import os
import zipfile
from collections import defaultdict

import numpy as np
import pandas as pd
import pytest
from test_gpu_residual_e2e import B, A, _run, trained  # noqa: F401  (trained: the module's fixture, made again for this module)

from yacht_amd import cohort, residual, sigio, synth
from yacht_amd.engine import RefDB
from yacht_amd.hypothesis_recovery_src import hyp_test_native

pytestmark = pytest.mark.gpu


def _files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _sub, fs in os.walk(root) for f in fs)


def _same_tree(a, b, what):
    names = _files_under(a)
    assert names == _files_under(b) and names, what
    for name in names:
        pa, pb = os.path.join(a, name), os.path.join(b, name)
        if name.endswith(residual.RESIDUAL_NAME):
            sa, sb = sigio.load_file_as_signatures(pa, ksize=31), sigio.load_file_as_signatures(pb, ksize=31)
            assert len(sa) == len(sb) == 1 and sa[0].name == sb[0].name and sa[0].md5sum() == sb[0].md5sum(), (what, name)
            assert np.array_equal(sa[0].minhash.mins, sb[0].minhash.mins), (what, name)
            assert np.array_equal(sa[0].minhash.abundances, sb[0].minhash.abundances), (what, name)
        elif name.endswith(".xlsx"):
            with zipfile.ZipFile(pa) as za, zipfile.ZipFile(pb) as zb:
                assert za.namelist() == zb.namelist(), (what, name)
                for entry in za.namelist():
                    assert za.read(entry) == zb.read(entry), (what, name, entry)
        else:
            with open(pa, "rb") as fa, open(pb, "rb") as fb:
                assert fa.read() == fb.read(), (what, name)
    return names


def _both_ways(cfg, files, tmp_path, monkeypatch, opts, what):
    """The cohort by default (the device's batched pass) and with every sample on the host-form path; the host-form calls of
    each are counted."""
    calls = {}
    real = residual.explain_call_sets
    res = {}
    for mode in ("device", "host"):
        count = []
        monkeypatch.setattr(residual, "explain_call_sets", lambda *a, _c=count, **k: (_c.append(1), real(*a, **k))[1])
        if mode == "host":
            monkeypatch.setenv("YACHT_COHORT_EXPLAIN", "host")
        else:
            monkeypatch.delenv("YACHT_COHORT_EXPLAIN", raising=False)
        res[mode] = _run(cfg, files, tmp_path / mode, *opts)
        calls[mode] = len(count)
    monkeypatch.delenv("YACHT_COHORT_EXPLAIN", raising=False)
    monkeypatch.setattr(residual, "explain_call_sets", real)
    names = _same_tree(str(res["device"]), str(res["host"]), what)
    return res["device"], names, calls


def _flat_copy(src, dst, name):
    sig = sigio.load_file_as_signatures(str(src), ksize=31)[0]
    sigio.write_sig_zip([sigio.make_signature(sig.minhash.mins, ksize=31, scaled=1000, name=name)], str(dst))
    return dst


NINE = ["0.9", "0.8", "0.7", "0.6", "0.5", "0.4", "0.3", "0.2", "0.1"]


@pytest.mark.parametrize("case", ["three_coverages_middle", "nine_coverages_two_passes", "with_abundance", "mixed_tracked_and_flat", "all_flat"])
def test_cohort_files_equal_the_host_form_path(trained, tmp_path, monkeypatch, case):
    tmp, cfg3, cfg4, sketch, files = trained
    names = ["mix", "second", "none"]  # (none: no overlap, no results folder, zeros in cohort_samples.tsv)
    if case == "three_coverages_middle":
        opts = ["--residual", "--min_coverage_list", "1", "0.5", "0.1", "--residual_coverage", "0.5"]
    elif case == "nine_coverages_two_passes":  # (1.0 is not listed: the forced coverage in front is no call set)
        opts = ["--residual", "--min_coverage_list", *NINE, "--residual_coverage", "0.1"]
    elif case == "with_abundance":
        opts = ["--residual", "--abundance", "--min_coverage_list", "1", "0.1"]
    else:
        opts = ["--residual", "--min_coverage_list", "0.5", "0.1"]
    paths = [files[n] for n in names]
    if case == "mixed_tracked_and_flat":
        paths = [files["mix_flat"], files["second"], files["none"]]
    elif case == "all_flat":
        paths = [files["mix_flat"], _flat_copy(files["second"], tmp_path / "second_flat.sig.zip", "second flat")]
    res, listed, calls = _both_ways(cfg3, paths, tmp_path, monkeypatch, opts, case)
    with_overlap = 2
    assert calls["device"] == 0 and calls["host"] == with_overlap  # no host-form call is left on the default path
    stems = [cohort.sample_stem(str(p)) for p in paths]
    for stem in stems[:with_overlap]:
        assert f"{stem}/{residual.EXPLAINED_NAME}" in listed and f"{stem}/{residual.RESIDUAL_NAME}" in listed
        got = pd.read_csv(res / stem / residual.EXPLAINED_NAME, sep="\t")
        n_cov = {"three_coverages_middle": 3, "nine_coverages_two_passes": 9}.get(case, 2)
        assert len(got) == n_cov and (got["num_hashes_explained"] > 100).all()
        assert (got["num_hashes_unexplained"] > 2000).all() == stem.startswith("mix")  # (D's hashes; `second` is all B and C)
        assert (got["num_hashes_in_database"] >= got["num_hashes_explained"]).all()
        flat = case == "all_flat" or (case == "mixed_tracked_and_flat" and stem == "mix_flat")
        assert (got["abund_explained"] == got["num_hashes_explained"]).all() == flat, (case, stem)
    summary = pd.read_csv(res / "cohort_samples.tsv", sep="\t").set_index("stem")
    assert (summary.loc[stems[:with_overlap], "f_hashes_explained"] > 0.1).all()
    if "none" in stems:
        assert summary.loc["none", "status"] == "no_overlap" and summary.loc["none", "f_hashes_explained"] == 0.0
        assert not (res / "none").exists()


def test_duplicate_names_take_the_host_form_for_the_recomputed_sample_only(trained, tmp_path, monkeypatch):
    """A takes B's organism name: the sample of B pulls A's row in by name, its tables are recomputed on the host and its
    residual takes the host-form call; the other sample's comes from the block's pass."""
    tmp, cfg3, cfg4, sketch, files = trained
    conf = json.load(open(cfg4))
    man = pd.read_csv(conf["manifest_file_path"], sep="\t")
    man.loc[man["organism_name"] == A, "organism_name"] = B
    dup_man = tmp_path / "dup_manifest.tsv"
    man.to_csv(dup_man, sep="\t", index=False)
    conf["manifest_file_path"] = str(dup_man)
    dup_cfg = tmp_path / "dup_config.json"
    dup_cfg.write_text(json.dumps(conf))
    opts = ["--residual", "--abundance", "--min_coverage_list", "1", "0.2", "--show_all"]
    res, listed, calls = _both_ways(dup_cfg, [files["b_twice"], files["mix"]], tmp_path, monkeypatch, opts, "duplicate names")
    # a sample was recomputed exactly when its tables list more organisms than it overlaps (rows pulled in by name)
    summary = pd.read_csv(res / "cohort_samples.tsv", sep="\t").set_index("stem")
    recomputed = []
    for stem in ("b_twice", "mix"):
        df = pd.read_csv(res / stem / "result_all.txt", sep="\t")
        if int((df["min_coverage"] == 1.0).sum()) != int(summary.loc[stem, "n_overlapping"]):
            recomputed.append(stem)
    assert "b_twice" in recomputed  # B's name selects two manifest rows, and b_twice overlaps one of them
    assert calls == {"device": len(recomputed), "host": 2}
    df = pd.read_csv(res / "b_twice" / "result_all.txt", sep="\t")
    assert len(df[(df["organism_name"] == B) & (df["min_coverage"] == 1.0)]) == 2


# ---- cohort._Device ----------------------------------------------------------------------------------------------------------
def _synthetic(n_samples, seed=31):
    values, offsets, _ = synth.config3_like(seed=21, n_refs=1500, n_sample=1000, n_present=10)
    refs = [values[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
    rng = np.random.default_rng(seed)
    samples, abunds = [], []
    for s in range(n_samples):
        present = rng.choice(len(refs), size=8, replace=False)
        cov = rng.choice([0.03, 0.2, 0.6, 1.0], size=8)  # some below the presence threshold, some that only a low min_coverage accepts
        samples.append(synth.sample_from_refs(rng, refs, present, cov, 6000))
        abunds.append(None if s % 3 == 0 else rng.integers(1, 500, samples[-1].size).astype(np.uint32))
    samples[5] = np.setdiff1d(np.unique(rng.integers(0, synth.max_hash_for_scaled(1000), 500, dtype=np.uint64)), values)
    samples[7] = np.zeros(0, np.uint64)
    for s in (5, 7):
        abunds[s] = None if abunds[s] is None else np.ones(samples[s].size, np.uint32)
    return values, offsets, samples, abunds


def _check_block_residual(db, block, abunds, got, covs, n_user, what):
    """flags / totals of collect() against residual.explain_call_sets on the call sets of the block's own present rows."""
    rows, _pv, pres, _ncov = got[:4]
    x_flags, x_totals = got[-1]
    first = len(covs) - n_user
    passes = (n_user + 6) // 7
    offs = np.concatenate([[0], np.cumsum([s.size for s in block])])
    assert x_flags.shape == (passes, offs[-1]) and x_totals.shape == (passes, len(block), 8, 2) and x_totals.dtype == np.uint64
    n_called = 0
    for s, sample in enumerate(block):
        sel = rows[:, 0] == s
        call_sets = [rows[sel, 1][pres[first + c, sel] != 0].astype(np.int64) for c in range(n_user)]
        n_called += sum(c.size for c in call_sets)
        ab = None if abunds is None else abunds[s]
        flags, totals = residual.explain_call_sets(db, sample, ab, call_sets)
        for c in range(n_user):
            assert np.array_equal(x_flags[c // 7, offs[s]:offs[s + 1]], flags[c]), (what, s, c)
            assert np.array_equal(x_totals[c // 7, s], totals[c]), (what, s, c)
    return n_called


@pytest.mark.parametrize("covs,n_user", [([1.0, 0.5, 0.05], 3), ([1.0] + [float(c) for c in NINE], 9)])
def test_device_blocks_against_the_host_form(hip_lib, covs, n_user):
    """Two blocks back to back on one _Device, the second smaller (65 samples, then 20); abundances for two samples in three."""
    values, offsets, samples, abunds = _synthetic(85)
    with RefDB(values, offsets) as db:
        n_max = int(np.max(db.sizes))
        tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        dev = cohort._Device(db, covs, 31, 0.95, tab[5], residual_sets=n_user)
        timer = defaultdict(float)
        for lo, hi in ((0, 65), (65, 85)):
            got = dev.collect(dev.launch(samples[lo:hi], None, abunds[lo:hi]), timer)
            assert len(got) == 5
            called = _check_block_residual(db, samples[lo:hi], abunds[lo:hi], got, covs, n_user, f"block {lo}")
            assert called > 20
            per_cov = [int((got[2][len(covs) - n_user + c] != 0).sum()) for c in range(n_user)]
            assert per_cov[-1] > per_cov[0] > 0  # the call sets differ between the coverages
        assert timer["dense_fallback_blocks"] == 0 and timer["gpu_explain"] > 0
        # without explain_abunds every hash counts once; an object without the pass returns what it always did
        got = dev.collect(dev.launch(samples[:9]), timer)
        _check_block_residual(db, samples[:9], None, got, covs, n_user, "no abundances")
        assert np.array_equal(got[-1][1][..., 0], got[-1][1][..., 1])
        plain = cohort._Device(db, covs, 31, 0.95, tab[5])
        assert len(plain.collect(plain.launch(samples[:9]), timer)) == 4


def test_device_dense_fallback_reruns_the_residual(hip_lib):
    values, offsets, samples, abunds = _synthetic(50)
    covs = [1.0, 0.1]
    with RefDB(values, offsets) as db:
        n_max = int(np.max(db.sizes))
        tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        dev = cohort._Device(db, covs, 31, 0.95, tab[5], cap=64, residual_sets=2)
        timer = defaultdict(float)
        first = dev.collect(dev.launch(samples[:30], None, abunds[:30]), timer)
        assert first[0].shape[0] > 64 and timer["dense_fallback_blocks"] == 1 and dev.cap > first[0].shape[0]
        assert _check_block_residual(db, samples[:30], abunds[:30], first, covs, 2, "dense") > 20
        second = dev.collect(dev.launch(samples[30:50], None, abunds[30:50]), timer)
        assert timer["dense_fallback_blocks"] == 1
        assert _check_block_residual(db, samples[30:50], abunds[30:50], second, covs, 2, "compact after growth") > 10
