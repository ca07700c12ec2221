"""`yacht run --abundance` from sequence to tables, on the GPU.

The database is `yacht sketch ref` + `yacht train` over the four GCF_*_genomic.fna.gz fixtures (unrelated genomes: at
scaled = 1000 a pair of them shares one hash or none, so training keeps all four).  The pair checked is
A = GCF_018918045.1 and B = GCF_018918235.1, which share no hash: a sample holding A's records three times and B's once
must report A and B present with median depths 3.0 and 1.0 and relative abundances 0.75 and 0.25, exactly -- the medians
do not move for the one k-mer of A's sketch and the three of B's that the genomes repeat internally.  (The other two
genomes appear in the unfiltered tables with the one or two hashes they share with A or B, and are not present.)  Then
the same through the cohort driver, the duplicate-organism-name path and the dense-fallback block."""
import gzip
import json
import os
import shutil
from collections import defaultdict

import numpy as np
import pandas as pd
import pytest

from yacht_amd import abundance, cli, cohort, sigio, synth
from yacht_amd import hypothesis_recovery_src as hr
from yacht_amd.engine import RefDB

pytestmark = pytest.mark.gpu

FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")
GENOMES = ["GCF_018918045.1_genomic", "GCF_018918095.1_genomic", "GCF_018918185.1_genomic", "GCF_018918235.1_genomic"]
A, B, C_, D = GENOMES[0], GENOMES[3], GENOMES[1], GENOMES[2]
REL, TINY = 1e-12, 1e-250  # tests/test_gpu_cohort.py
DIVIDED = ("p_vals", "actual_confidence_with_coverage", "alt_confidence_mut_rate_with_coverage", "abund_mean_overlap",
           "abund_mean_exclusive", "f_weighted_overlap", "relative_abundance")


def _fasta(path, parts):
    """A plain FASTA holding the records of each (genome, copies) of parts, `copies` times."""
    with open(path, "wb") as out:
        for genome, copies in parts:
            with gzip.open(os.path.join(FX, genome + ".fna.gz"), "rb") as f:
                text = f.read()
            if not text.endswith(b"\n"):
                text += b"\n"
            out.write(text * copies)
    return path


@pytest.fixture(scope="module")
def trained(hip_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("abund_e2e")
    gdir = tmp / "genomes"
    gdir.mkdir()
    for g in GENOMES:
        shutil.copyfile(os.path.join(FX, g + ".fna.gz"), gdir / (g + ".fna.gz"))
    ref_zip = tmp / "refs.sig.zip"
    cli.main(["sketch", "ref", "--infile", str(gdir), "--kmer", "31", "--scaled", "1000", "--outfile", str(ref_zip)])
    out = tmp / "db"
    out.mkdir()
    assert cli.main(["train", "--ref_file", str(ref_zip), "--ksize", "31", "--prefix", "db", "--ani_thresh", "0.95",
                     "--outdir", str(out), "--num_threads", "2", "--force"]) == 0
    cfg = out / "db_config.json"
    man = pd.read_csv(json.load(open(cfg))["manifest_file_path"], sep="\t")
    assert sorted(man["organism_name"]) == sorted(GENOMES)  # training kept all four
    smp = tmp / "samples"
    smp.mkdir()
    for name, parts in (("three_to_one", [(A, 3), (B, 1)]), ("one_to_one", [(C_, 1), (D, 1)]), ("b_twice", [(B, 2)])):
        cli.main(["sketch", "sample", "--infile", str(_fasta(tmp / f"{name}.fa", parts)), "--kmer", "31", "--scaled", "1000",
                  "--outfile", str(smp / f"{name}.sig.zip")])
    refs = sigio.load_file_as_signatures(str(ref_zip), ksize=31)
    held = np.concatenate([np.asarray(r.minhash.mins, np.uint64) for r in refs])
    rng = np.random.default_rng(12)
    none = np.setdiff1d(np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 3000, dtype=np.uint64)), held)
    sigio.write_sig_zip([sigio.make_signature(none, ksize=31, scaled=1000, name="none", abundances=1 + rng.integers(0, 9, none.size))],
                        str(smp / "none.sig.zip"))
    return tmp, cfg, [smp / f"{n}.sig.zip" for n in ("three_to_one", "one_to_one", "none", "b_twice")]


def _run(cfg, files, outdir, *opts):
    outdir.mkdir()
    assert cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(outdir), *opts]) == 0
    return outdir / "results"


def test_three_to_one_mix_from_sequence(trained, tmp_path):
    tmp, cfg, files = trained
    res = _run(cfg, files[:1], tmp_path / "with", "--abundance", "--min_coverage_list", "1")
    df = pd.read_csv(res / "result_all.txt", sep="\t")
    assert list(df.columns[-7:]) == abundance.ABUNDANCE_COLUMNS and list(df.columns[-15:-7]) == hr.GIVEN_COLUMNS
    assert set(df["organism_name"]) >= {A, B}
    assert sorted(df[df["in_sample_est"]]["organism_name"]) == sorted([A, B])
    assert (df[~df["in_sample_est"]]["relative_abundance"] == 0.0).all() and (df[~df["in_sample_est"]]["num_matches"] <= 2).all()
    a, b = df[df["organism_name"] == A].iloc[0], df[df["organism_name"] == B].iloc[0]
    print("medians", a["abund_median_exclusive"], b["abund_median_exclusive"], "relative", a["relative_abundance"],
          b["relative_abundance"], "means", a["abund_mean_exclusive"], b["abund_mean_exclusive"])
    assert a["abund_median_exclusive"] == 3.0 and b["abund_median_exclusive"] == 1.0
    assert a["relative_abundance"] == 0.75 and b["relative_abundance"] == 0.25
    for r in (a, b):
        assert r["abund_mean_exclusive"] >= r["abund_median_exclusive"] and r["abund_mean_overlap"] >= r["abund_median_exclusive"]
        assert r["abund_sum_overlap"] >= r["abund_sum_exclusive"] >= r["num_matches"] > 2000
        assert r["num_matches"] == r["num_exclusive_kmers_to_genome"]
    assert abs(a["f_weighted_overlap"] + b["f_weighted_overlap"] - 1.0) < 1e-12  # the sample holds nothing else, A and B share nothing
    prof = pd.read_csv(res / abundance.PROFILE_NAME, sep="\t")
    assert list(prof.columns) == abundance.PROFILE_COLUMNS
    assert prof["organism_name"].tolist() == [A, B] and prof["relative_abundance"].tolist() == [0.75, 0.25]
    assert prof["abund_median_exclusive"].tolist() == [3.0, 1.0] and prof["min_coverage"].tolist() == [1.0, 1.0]
    sheet = pd.read_csv(res / "sheets" / "min_coverage1.0.tsv", sep="\t")
    assert list(sheet.columns) == list(df.columns) and sheet["organism_name"].tolist() == df[df["in_sample_est"]]["organism_name"].tolist()
    # the same run without the flag: the tables as they were (manifest columns + the eight), and no profile
    plain = _run(cfg, files[:1], tmp_path / "without", "--min_coverage_list", "1")
    pf = pd.read_csv(plain / "result_all.txt", sep="\t")
    assert list(pf.columns) == list(df.columns[:-7]) and list(pf.columns[-8:]) == hr.GIVEN_COLUMNS
    assert pf.astype(str).equals(df[pf.columns].astype(str))
    assert sorted(os.listdir(plain)) == ["result.xlsx", "result_all.txt", "sheets"]
    assert sorted(os.listdir(res)) == sorted(["result.xlsx", "result_all.txt", "sheets", abundance.PROFILE_NAME])


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    tiny = (np.abs(got) < TINY) & (np.abs(want) < TINY)
    return both_nan | tiny | (np.abs(got - want) <= REL * np.abs(want))


def _same_table(a, b, what):
    assert list(a.columns) == list(b.columns) and len(a) == len(b), what
    for c in a.columns:
        if c in DIVIDED:
            assert _close(a[c].astype(float), b[c].astype(float)).all(), (what, c)
        else:  # names, counts, sums, the median: exact
            assert a[c].astype(str).tolist() == b[c].astype(str).tolist(), (what, c)


def _same_results(cdir, sdir, what):
    names = ["result_all.txt", abundance.PROFILE_NAME] + [os.path.join("sheets", s) for s in sorted(os.listdir(sdir / "sheets"))]
    assert sorted(os.listdir(cdir / "sheets")) == sorted(os.listdir(sdir / "sheets")), what
    for n in names:
        _same_table(pd.read_csv(cdir / n, sep="\t", dtype=str), pd.read_csv(sdir / n, sep="\t", dtype=str), f"{what} {n}")


def test_cohort_equals_single_runs(trained, tmp_path):
    tmp, cfg, files = trained
    opts = ["--min_coverage_list", "1", "0.5", "0.05", "--show_all"]
    files = files[:3]
    res = _run(cfg, files, tmp_path / "cohort", "--abundance", *opts)
    assert not (res / "none").exists()
    for f in files[:2]:
        stem = cohort.sample_stem(str(f))
        _same_results(res / stem, _run(cfg, [f], tmp_path / f"single_{stem}", "--abundance", *opts), stem)
    with pytest.raises(SystemExit):  # the single path stops at an empty multisearch result
        _run(cfg, files[2:], tmp_path / "single_none", "--abundance", *opts)
    pres = pd.read_csv(res / "cohort_presence.tsv", sep="\t")
    assert list(pres.columns) == cohort.PRESENCE_COLUMNS + ["abund_median_exclusive", "relative_abundance"]
    top = pres[(pres["sample"] == "three_to_one") & (pres["min_coverage"] == 1.0)].set_index("organism_name")
    assert top.loc[A, "abund_median_exclusive"] == 3.0 and top.loc[B, "abund_median_exclusive"] == 1.0
    assert top.loc[A, "relative_abundance"] == 0.75 and top.loc[B, "relative_abundance"] == 0.25
    even = pres[(pres["sample"] == "one_to_one") & (pres["min_coverage"] == 1.0)]
    assert sorted(even["organism_name"]) == sorted([C_, D]) and even["relative_abundance"].tolist() == [0.5, 0.5]
    assert even["abund_median_exclusive"].tolist() == [1.0, 1.0]
    # the same cohort without the flag: the old header, the old tables, no profile
    plain = _run(cfg, files, tmp_path / "cohort_plain", *opts)  # (files: the three above)
    assert list(pd.read_csv(plain / "cohort_presence.tsv", sep="\t").columns) == cohort.PRESENCE_COLUMNS
    for f in files[:2]:
        stem = cohort.sample_stem(str(f))
        assert sorted(os.listdir(plain / stem)) == ["result.xlsx", "result_all.txt", "sheets"]
        got = pd.read_csv(plain / stem / "result_all.txt", sep="\t", dtype=str)
        want = pd.read_csv(res / stem / "result_all.txt", sep="\t", dtype=str)
        assert list(got.columns) == list(want.columns[:-7]) and list(got.columns[-8:]) == hr.GIVEN_COLUMNS
        assert got.equals(want[got.columns])


def test_duplicate_names_get_the_columns_too(trained, tmp_path):
    """A reference without overlap that shares its organism name with one that has it enters the tables by name: its sums
    are 0, its means and median NaN, in the cohort as in the single path.  The sample is B twice, which shares no hash
    with A; A takes B's name."""
    tmp, cfg, files = trained
    conf = json.load(open(cfg))
    man = pd.read_csv(conf["manifest_file_path"], sep="\t")
    man.loc[man["organism_name"] == A, "organism_name"] = B
    dup_man = tmp_path / "dup_manifest.tsv"
    man.to_csv(dup_man, sep="\t", index=False)
    conf["manifest_file_path"] = str(dup_man)
    dup_cfg = tmp_path / "dup_config.json"
    dup_cfg.write_text(json.dumps(conf))
    opts = ["--abundance", "--min_coverage_list", "1", "--show_all"]
    res = _run(dup_cfg, [files[3], files[1]], tmp_path / "cohort", *opts)
    single = _run(dup_cfg, [files[3]], tmp_path / "single", *opts)
    _same_results(res / "b_twice", single, "duplicate names")
    df = pd.read_csv(single / "result_all.txt", sep="\t")
    extra = df[df["abund_sum_overlap"] == 0]
    assert len(extra) == 1 and len(df) >= 3 and extra["organism_name"].iloc[0] == B and not extra["in_sample_est"].iloc[0]
    assert extra["abund_sum_exclusive"].iloc[0] == 0 and extra["relative_abundance"].iloc[0] == 0.0
    assert extra[["abund_mean_overlap", "abund_mean_exclusive", "abund_median_exclusive"]].isna().all().all()
    hit = df[df["in_sample_est"]]
    assert hit["organism_name"].tolist() == [B] and hit["abund_median_exclusive"].tolist() == [2.0]
    assert hit["relative_abundance"].tolist() == [1.0]


def test_block_values_compact_and_dense(hip_lib):
    """The values a block gathers at its rows equal RefDB.abundance of every sample, for compact rows and for the block
    that falls back to the dense counts."""
    values, offsets, _ = synth.config3_like(seed=21, n_refs=2000, n_sample=1000, n_present=10)
    refs = [values[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
    rng = np.random.default_rng(6)
    samples = [synth.real_shape_sample(rng, refs, n_sample=1500, frac_overlapping=0.05) for _ in range(40)]
    abunds = [rng.integers(1, 50, s.size).astype(np.uint32) for s in samples]
    covs = [1.0, 0.1]
    with RefDB(values, offsets) as db:
        n_max = int(np.max(db.sizes))
        tab = hr.hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        dev = cohort._Device(db, covs, 31, 0.95, tab[5], cap=64, abund_samples=30)
        timer = defaultdict(float)
        for lo, hi, dense in ((0, 30, 1), (30, 40, 1)):
            got = dev.collect(dev.launch(samples[lo:hi], abunds[lo:hi]), timer)
            assert timer["dense_fallback_blocks"] == dense and timer["gpu_abund"] > 0 and len(got) == 5
            rows = got[0]
            assert rows.shape[0] > 64 or lo
            for s in range(hi - lo):
                sel = rows[:, 0] == s
                w_ov, w_m, med = db.abundance(samples[lo + s], abunds[lo + s])
                ref = rows[sel, 1]
                assert np.array_equal(ref, np.flatnonzero(w_ov)) and ref.size
                assert np.array_equal(got[4][0][sel], w_ov[ref]) and np.array_equal(got[4][1][sel], w_m[ref]), (lo, s)
                assert np.array_equal(got[4][2][sel], med[ref]), (lo, s)
