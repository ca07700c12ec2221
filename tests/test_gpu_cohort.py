"""`yacht run` over a cohort (yacht_amd/cohort.py) and the device presence test (yh_presence_rows_device), on the GPU:
per-sample results equal single-sample runs of the same files, block boundaries against the oracle, the kernel against the
reference's own hypothesis-test outputs, and duplicate organism names."""
import json
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from oracle import oracle
from yacht_amd import cli, cohort, sigio, synth, xlsx
from yacht_amd.engine import RefDB
from yacht_amd.hypothesis_recovery_src import hyp_test_batch, hyp_test_native

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FX = os.path.join(GOLD, "fixtures")
REL, TINY = 1e-12, 1e-250  # tests/test_hyp_native.py
FLOAT_COLS = ("p_vals", "actual_confidence_with_coverage", "alt_confidence_mut_rate_with_coverage",
              "actual_confidence_wo_coverage", "alt_confidence_mut_rate_wo_coverage")


def close(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    tiny = (np.abs(got) < TINY) & (np.abs(want) < TINY)
    return tiny | (np.abs(got - want) <= REL * np.abs(want))


def _same_table(a: pd.DataFrame, b: pd.DataFrame, what: str) -> None:
    assert list(a.columns) == list(b.columns), what
    assert len(a) == len(b), what
    for c in a.columns:
        if c in FLOAT_COLS:
            assert close(a[c].astype(float), b[c].astype(float)).all(), (what, c)
        else:
            assert a[c].astype(str).tolist() == b[c].astype(str).tolist(), (what, c)


def _same_results(cohort_dir, single_dir, what):
    _same_table(pd.read_csv(cohort_dir / "result_all.txt", sep="\t", dtype=str), pd.read_csv(single_dir / "result_all.txt", sep="\t", dtype=str),
                f"{what} result_all")
    sheets = sorted(os.listdir(single_dir / "sheets"))
    assert sorted(os.listdir(cohort_dir / "sheets")) == sheets, what
    for s in sheets:
        _same_table(pd.read_csv(cohort_dir / "sheets" / s, sep="\t", dtype=str), pd.read_csv(single_dir / "sheets" / s, sep="\t", dtype=str),
                    f"{what} {s}")
    assert list(xlsx.read_xlsx(str(cohort_dir / "result.xlsx"))) == list(xlsx.read_xlsx(str(single_dir / "result.xlsx"))), what


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cohort")
    out = tmp / "db"
    out.mkdir()
    ref_zip = tmp / "20_genomes_sketches.zip"
    shutil.copyfile(os.path.join(FX, "20_genomes_sketches.zip"), ref_zip)
    assert cli.main(["train", "--ref_file", str(ref_zip), "--ksize", "31", "--prefix", "db", "--ani_thresh", "0.95",
                     "--outdir", str(out), "--num_threads", "2", "--force"]) == 0
    # five samples from the fixture sample: itself, hash subsets with other abundances, one with no overlap
    base = sigio.load_file_as_signatures(os.path.join(FX, "sample.sig.zip"), ksize=31)[0].minhash
    mins = np.asarray(base.mins, dtype=np.uint64)
    ab = np.asarray(base.abundances, dtype=np.int64)
    smp = tmp / "samples"
    smp.mkdir()
    shutil.copyfile(os.path.join(FX, "sample.sig.zip"), smp / "full.sig.zip")
    rng = np.random.default_rng(9)
    # the fixture sample shares few hashes with the references: every subset keeps some of those
    refs = sigio.load_file_as_signatures(str(ref_zip), ksize=31)
    shared = np.flatnonzero(np.isin(mins, np.concatenate([np.asarray(r.minhash.mins, np.uint64) for r in refs])))
    assert shared.size >= 2
    idx = np.arange(mins.size)
    for name, keep, abund in (("half", (idx % 2 == 0) | np.isin(idx, shared), lambda a: a * 3),
                              ("fifth", (idx % 5 == 1) | np.isin(idx, shared[:1]), lambda a: np.ones_like(a)),
                              ("thirds", (idx % 3 == 0) | np.isin(idx, shared), lambda a: 1 + a % 4)):
        sigio.write_sig_zip([sigio.make_signature(mins[keep], ksize=31, scaled=1000, name=name, abundances=abund(ab[keep]))],
                            str(smp / f"{name}.sig.zip"))
    none = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 3000, dtype=np.uint64))
    none = np.setdiff1d(none, mins)
    sigio.write_sig_zip([sigio.make_signature(none, ksize=31, scaled=1000, name="none", abundances=np.ones(none.size, np.int64))],
                        str(smp / "none.sig.zip"))
    files = [smp / f"{n}.sig.zip" for n in ("full", "half", "fifth", "thirds", "none")]
    return tmp, out / "db_config.json", files


@pytest.mark.parametrize("opts", [["--keep_raw"], ["--min_coverage_list", "0.05", "0.001", "--show_all"]])
def test_fixture_cohort_equals_single_runs(hip_lib, trained, tmp_path, monkeypatch, opts):
    tmp, cfg, files = trained
    cdir = tmp_path / "cohort"
    cdir.mkdir()
    before = sorted(p.name for p in files[0].parent.iterdir())
    assert cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(cdir), *opts]) == 0
    assert sorted(p.name for p in files[0].parent.iterdir()) == before  # no sample_<stem>_intermediate_files
    res = cdir / "results"
    summ = pd.read_csv(res / "cohort_samples.tsv", sep="\t")
    assert summ["stem"].tolist() == ["full", "half", "fifth", "thirds", "none"]
    assert summ["status"].tolist() == ["ok"] * 4 + ["no_overlap"] and int(summ["n_overlapping"].iloc[-1]) == 0
    assert not (res / "none").exists()
    pres = pd.read_csv(res / "cohort_presence.tsv", sep="\t")
    assert list(pres.columns) == cohort.PRESENCE_COLUMNS
    for native in ("0", "1"):
        monkeypatch.setenv("YACHT_HYP_NATIVE", native)
        for f in files[:4]:
            stem = cohort.sample_stem(str(f))
            sdir = tmp_path / f"single_{native}_{stem}"
            sdir.mkdir()
            assert cli.main(["run", "--json", str(cfg), "--sample_file", str(f), "--num_threads", "2", "--outdir", str(sdir), *opts]) == 0
            _same_results(res / stem, sdir / "results", f"{stem} native={native}")
            single = pd.read_csv(sdir / "results" / "result_all.txt", sep="\t")
            want = single[single["in_sample_est"] == True]  # noqa: E712
            got = pres[pres["sample"] == stem]
            assert got["organism_name"].tolist() == want["organism_name"].tolist()
            assert got["num_matches"].tolist() == want["num_matches"].tolist()


def _device_for(db, covs, ksize=31, sig=0.99, ani=0.95, n_max=None):
    n_max = int(np.max(db.sizes)) if n_max is None else n_max
    tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), ksize, sig, ani, 1.0)
    return cohort._Device(db, covs, ksize, ani, tab[5]), tab


def _check_block(values, offsets, block, got, tab, covs, what):
    """A block's rows against the oracle's counts, its decisions against hyp_test_batch, for every sample of it."""
    rows, pv, pres, ncov = got
    assert np.array_equal(np.lexsort((rows[:, 0], rows[:, 1])), np.arange(rows.shape[0])), what  # (reference, sample) order
    for s in range(len(block)):
        sel = rows[:, 0] == s
        want_ov = oracle.overlap(values, offsets, block[s], threads=4)
        want_e, want_m = oracle.exclusive(values, offsets, want_ov > 0, block[s])
        hit = np.flatnonzero(want_ov)
        assert np.array_equal(rows[sel, 1], hit), (what, s)
        assert np.array_equal(rows[sel, 2], want_ov[hit]) and np.array_equal(rows[sel, 3], want_e[hit]), (what, s)
        assert np.array_equal(rows[sel, 4], want_m[hit]), (what, s)
        for c, cov in enumerate(covs):
            w = hyp_test_batch(want_e[hit], want_m[hit], 31, 0.99, 0.95, cov)
            assert np.array_equal(pres[c, sel].astype(bool), w[0]) and np.array_equal(ncov[c, sel], w[3]), (what, s, cov)
            assert np.array_equal(tab[5][ncov[c, sel]], w[5]), (what, s, cov)
            assert close(pv[c, sel], w[1]).all(), (what, s, cov)


def _sample_rows(got, s):
    sel = got[0][:, 0] == s
    return got[0][sel, 1:], got[1][:, sel], got[2][:, sel], got[3][:, sel]


def _synthetic(n_samples):
    values, offsets, _ = synth.config3_like(seed=21, n_refs=2000, n_sample=1000, n_present=10)
    refs = [values[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
    rng = np.random.default_rng(4)
    samples = [synth.real_shape_sample(rng, refs, n_sample=1500, frac_overlapping=0.05) for _ in range(n_samples)]
    samples[17] = np.setdiff1d(np.unique(rng.integers(0, synth.max_hash_for_scaled(1000), 500, dtype=np.uint64)), values)
    return values, offsets, samples


def test_block_boundary_against_oracle(hip_lib):
    """300 samples (two blocks) against ~2 000 references, one sample without overlap and one repeated across the block
    boundary: the rows against the oracle's counts and the decisions against hyp_test_batch, for every sample."""
    from collections import defaultdict

    values, offsets, samples = _synthetic(300)
    samples[260] = samples[3].copy()
    covs = [1.0, 0.5, 0.05]
    with RefDB(values, offsets) as db:
        dev, tab = _device_for(db, covs)
        timer = defaultdict(float)
        got = []
        for lo in (0, 256):
            block = samples[lo:lo + 256]
            got.append(dev.collect(dev.launch(block), timer))
            _check_block(values, offsets, block, got[-1], tab, covs, f"block at {lo}")
        assert timer["dense_fallback_blocks"] == 0  # (compact rows throughout)
    assert not (got[0][0][:, 0] == 17).any()
    # the repeated sample: sample 3 of the first block and sample 260 (4 of the second) give the same rows and results
    a, b = _sample_rows(got[0], 3), _sample_rows(got[1], 260 - 256)
    assert a[0].shape[0] > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_dense_fallback_when_the_rows_exceed_the_capacity(hip_lib):
    """A block with more compact rows than the buffers hold takes its rows from the dense counts (cohort._Device.collect),
    then the capacity grows and the next block is compact again: both against the oracle."""
    from collections import defaultdict

    values, offsets, samples = _synthetic(60)
    covs = [1.0, 0.1]
    with RefDB(values, offsets) as db:
        n_max = int(np.max(db.sizes))
        tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        dev = cohort._Device(db, covs, 31, 0.95, tab[5], cap=64)
        timer = defaultdict(float)
        first = dev.collect(dev.launch(samples[:30]), timer)
        assert first[0].shape[0] > 64 and timer["dense_fallback_blocks"] == 1 and dev.cap > first[0].shape[0]
        _check_block(values, offsets, samples[:30], first, tab, covs, "dense")
        second = dev.collect(dev.launch(samples[30:50]), timer)
        assert timer["dense_fallback_blocks"] == 1
        _check_block(values, offsets, samples[30:50], second, tab, covs, "compact after growth")


def _kernel(e, m, ksize, sig, ani, covs):
    """The presence kernel alone on rows (sample 0, ref i, -, e_i, m_i)."""
    import torch

    values, offsets = synth.pack([np.arange(1, 5, dtype=np.uint64)])
    with RefDB(values, offsets) as db:
        e = np.asarray(e, np.int64)
        dev, tab = _device_for(db, covs, ksize, sig, ani, n_max=int(e.max()))
        n = e.size
        rows = np.zeros((n, 5), np.int32)
        rows[:, 1] = np.arange(n)
        rows[:, 3] = e
        rows[:, 4] = np.asarray(m, np.int64)
        d_rows = torch.from_numpy(rows).to(dev.dev)
        d_n = torch.tensor([n], dtype=torch.int32, device=dev.dev)
        out = dev._out(n)
        dev.presence(d_rows, d_n.data_ptr(), n, out)
        db.synchronize()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out], tab


def test_kernel_on_the_reference_grid(hip_lib):
    with open(os.path.join(GOLD, "golden_hyp.json")) as f:
        grid = json.load(f)["single_hyp_test"]
    by = {}
    for r in grid:
        by.setdefault((r["k"], r["sig"], r["ani"]), []).append(r)
    for (k, sig, ani), rows in by.items():
        covs = sorted({r["cov"] for r in rows})
        (pv, pres, ncov), tab = _kernel([r["e"] for r in rows], [r["m"] for r in rows], k, sig, ani, covs)
        for i, r in enumerate(rows):
            c = covs.index(r["cov"])
            out = r["out"]
            assert bool(pres[c, i]) == out[0] and int(ncov[c, i]) == out[3], r
            assert tab[5][ncov[c, i]] == out[5], r
            assert close([pv[c, i]], [out[1]])[0] and close([tab[6][ncov[c, i]]], [out[6]])[0] and close([tab[7][ncov[c, i]]], [out[7]])[0], r


def test_kernel_on_the_real_tuples(hip_lib):
    z = np.load(os.path.join(GOLD, "golden_hyp_real.npz"))
    with open(os.path.join(GOLD, "golden_hyp_real.json")) as f:
        meta = json.load(f)
    for fi, par in enumerate(meta["files"]):
        for cov in (1.0, 0.1, 0.01):
            w = (z["file_index"] == fi) & (z["cov"] == cov)
            (pv, pres, ncov), tab = _kernel(z["e"][w], z["m"][w], par["ksize"], par["significance"], par["ani_thresh"], [cov])
            c, e = 0, z["e"][w]
            assert np.array_equal(pres[c].astype(bool), z["present"][w]), cov
            assert np.array_equal(ncov[c], z["n_cov"][w]), cov
            assert np.array_equal(tab[5][ncov[c]], z["thr"][w]), cov
            ok = close(pv[c], z["p_val"][w])
            assert ok.all(), (cov, e[~ok][:3], pv[c][~ok][:3], z["p_val"][w][~ok][:3])
            assert close(tab[6][ncov[c]], z["conf"][w]).all() and close(tab[7][ncov[c]], z["alt"][w]).all()


def test_duplicate_names_equal_single_path(hip_lib, trained, tmp_path):
    """Two references under one organism name: get_exclusive_hashes selects by name, so a reference without overlap can
    enter the subset; the cohort recomputes that sample's counts as the single path does."""
    tmp, cfg, files = trained
    conf = json.load(open(cfg))
    man = pd.read_csv(conf["manifest_file_path"], sep="\t")
    single = tmp_path / "probe"
    single.mkdir()
    assert cli.main(["run", "--json", str(cfg), "--sample_file", str(files[1]), "--num_threads", "2", "--outdir", str(single),
                     "--show_all"]) == 0
    hit = set(pd.read_csv(single / "results" / "result_all.txt", sep="\t")["organism_name"])
    have, miss = [n for n in man["organism_name"] if n in hit], [n for n in man["organism_name"] if n not in hit]
    assert have and miss
    man.loc[man["organism_name"] == miss[0], "organism_name"] = have[0]  # a non-overlapping reference takes an overlapping one's name
    dup_man = tmp_path / "dup_manifest.tsv"
    man.to_csv(dup_man, sep="\t", index=False)
    conf["manifest_file_path"] = str(dup_man)
    dup_cfg = tmp_path / "dup_config.json"
    dup_cfg.write_text(json.dumps(conf))
    cdir = tmp_path / "cohort"
    cdir.mkdir()
    assert cli.main(["run", "--json", str(dup_cfg), "--sample_file", *map(str, files[:3]), "--num_threads", "2", "--outdir",
                     str(cdir), "--show_all"]) == 0
    for f in files[:3]:
        stem = cohort.sample_stem(str(f))
        sdir = tmp_path / f"single_{stem}"
        sdir.mkdir()
        assert cli.main(["run", "--json", str(dup_cfg), "--sample_file", str(f), "--num_threads", "2", "--outdir", str(sdir),
                         "--show_all"]) == 0
        _same_results(cdir / "results" / stem, sdir / "results", stem)
