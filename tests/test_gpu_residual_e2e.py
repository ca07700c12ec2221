"""`yacht run --residual` from sequence to files, on the GPU.

The databases are `yacht sketch ref` + `yacht train` over the GCF_*_genomic.fna.gz fixtures (unrelated genomes: at
scaled = 1000 a pair of them shares a hash or two, or none): db3 holds A, B and C, db4 all four.  The sample holds A's
records three times, B's once, D's twice and the first 12 000 bases of C -- a dozen of C's ~3 000 sketch hashes, far
below any presence threshold, so that "in the database but not explained" is not an empty class.  Against db3, A and B
are called present; everything of D and the sliver of C is left over, and the left-over run against db4 finds D.
Every expected number comes from Python sets over the four reference sketches and the sample sketch."""
import gzip
import json
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from yacht_amd import abundance, cli, cohort, residual, sigio

pytestmark = pytest.mark.gpu

FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")
GENOMES = ["GCF_018918045.1_genomic", "GCF_018918095.1_genomic", "GCF_018918185.1_genomic", "GCF_018918235.1_genomic"]
A, B, C_, D = GENOMES[0], GENOMES[3], GENOMES[1], GENOMES[2]
SLIVER = 12_000  # bases of C's first record in the sample


def _records(genome):
    with gzip.open(os.path.join(FX, genome + ".fna.gz"), "rb") as f:
        text = f.read()
    return text if text.endswith(b"\n") else text + b"\n"


def _fasta(path, parts, sliver_of=None):
    """A plain FASTA holding the records of each (genome, copies) of parts `copies` times, and optionally the first
    SLIVER bases of the first record of one more genome."""
    with open(path, "wb") as out:
        for genome, copies in parts:
            out.write(_records(genome) * copies)
        if sliver_of is not None:
            lines = _records(sliver_of).split(b"\n")
            seq = b""
            for line in lines[1:]:
                if line.startswith(b">") or len(seq) >= SLIVER:
                    break
                seq += line
            out.write(b">sliver\n" + seq[:SLIVER] + b"\n")
    return path


def _train(tmp, prefix, genomes):
    gdir = tmp / f"genomes_{prefix}"
    gdir.mkdir()
    for g in genomes:
        shutil.copyfile(os.path.join(FX, g + ".fna.gz"), gdir / (g + ".fna.gz"))
    ref_zip = tmp / f"{prefix}_refs.sig.zip"
    cli.main(["sketch", "ref", "--infile", str(gdir), "--kmer", "31", "--scaled", "1000", "--outfile", str(ref_zip)])
    out = tmp / prefix
    out.mkdir()
    assert cli.main(["train", "--ref_file", str(ref_zip), "--ksize", "31", "--prefix", prefix, "--ani_thresh", "0.95",
                     "--outdir", str(out), "--num_threads", "2", "--force"]) == 0
    cfg = out / f"{prefix}_config.json"
    man = pd.read_csv(json.load(open(cfg))["manifest_file_path"], sep="\t")
    assert sorted(man["organism_name"]) == sorted(genomes)  # training kept all of them
    return cfg, ref_zip


@pytest.fixture(scope="module")
def trained(hip_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("residual_e2e")
    cfg3, _ = _train(tmp, "db3", [A, B, C_])
    cfg4, ref_zip = _train(tmp, "db4", GENOMES)
    sketch = {s.name: set(int(h) for h in s.minhash.mins) for s in sigio.load_file_as_signatures(str(ref_zip), ksize=31)}
    assert sorted(sketch) == sorted(GENOMES)
    smp = tmp / "samples"
    smp.mkdir()
    for name, parts, sliver in (("mix", [(A, 3), (B, 1), (D, 2)], C_), ("second", [(C_, 1), (B, 2)], None), ("b_twice", [(B, 2)], None)):
        cli.main(["sketch", "sample", "--infile", str(_fasta(tmp / f"{name}.fa", parts, sliver)), "--kmer", "31", "--scaled", "1000",
                  "--outfile", str(smp / f"{name}.sig.zip")])
    held = np.array(sorted(set().union(*sketch.values())), dtype=np.uint64)
    rng = np.random.default_rng(12)
    none = np.setdiff1d(np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 3000, dtype=np.uint64)), held)
    sigio.write_sig_zip([sigio.make_signature(none, ksize=31, scaled=1000, name="none", abundances=1 + rng.integers(0, 9, none.size))],
                        str(smp / "none.sig.zip"))
    # the mix again, as a sketch that tracks no abundances
    mix = sigio.load_file_as_signatures(str(smp / "mix.sig.zip"), ksize=31)[0]
    sigio.write_sig_zip([sigio.make_signature(mix.minhash.mins, ksize=31, scaled=1000, name=mix.name)], str(smp / "mix_flat.sig.zip"))
    files = {n: smp / f"{n}.sig.zip" for n in ("mix", "second", "none", "b_twice", "mix_flat")}
    return tmp, cfg3, cfg4, sketch, files


def _run(cfg, files, outdir, *opts):
    outdir.mkdir()
    assert cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(outdir), *opts]) == 0
    return outdir / "results"


def _read(path):
    """A table with its floats parsed exactly (the default parser may be one unit in the last place off)."""
    return pd.read_csv(path, sep="\t", float_precision="round_trip")


def _sample(path):
    mh = sigio.load_file_as_signatures(str(path), ksize=31)[0].minhash
    ab = mh.abundances if mh.abundances is not None else np.ones(len(mh), dtype=np.int64)
    return {int(h): int(a) for h, a in zip(mh.mins, ab)}, mh.abundances is not None


def _expected_row(cov, n_present, sample, known, explained):
    """One row of sample_explained.tsv from Python sets: sample = {hash: abundance}."""
    n, total = len(sample), sum(sample.values())
    in_db, ex = [h for h in sample if h in known], [h for h in sample if h in explained]
    a_db, a_ex = sum(sample[h] for h in in_db), sum(sample[h] for h in ex)
    return [cov, n_present, n, len(in_db), len(ex), n - len(ex), total, a_db, a_ex, total - a_ex,
            len(in_db) / n, len(ex) / n, a_db / total, a_ex / total]


def _check_residual(path, sample, tracked, explained, name):
    assert sigio.zip_has_manifest(str(path))
    sigs = sigio.load_file_as_signatures(str(path), ksize=31)
    assert len(sigs) == 1 and sigs[0].name == name and sigs[0].minhash.scaled == 1000 and sigs[0].minhash.ksize == 31
    mh = sigs[0].minhash
    left = sorted(h for h in sample if h not in explained)
    assert [int(h) for h in mh.mins] == left
    if tracked:
        assert [int(a) for a in mh.abundances] == [sample[h] for h in left]
    else:
        assert mh.abundances is None
    return left


def test_residual_of_a_mix_from_sequence(trained, tmp_path):
    tmp, cfg3, cfg4, sketch, files = trained
    res = _run(cfg3, [files["mix"]], tmp_path / "with", "--residual", "--abundance", "--min_coverage_list", "1", "0.1")
    df = pd.read_csv(res / "result_all.txt", sep="\t")
    for cov in (1.0, 0.1):
        assert sorted(df[(df["min_coverage"] == cov) & df["in_sample_est"]]["organism_name"]) == sorted([A, B]), cov
    sample, tracked = _sample(files["mix"])
    assert tracked and max(sample.values()) >= 3
    known = sketch[A] | sketch[B] | sketch[C_]
    explained = sketch[A] | sketch[B]
    got = _read(res / residual.EXPLAINED_NAME)
    assert list(got.columns) == residual.EXPLAINED_COLUMNS
    want = [_expected_row(1.0, 2, sample, known, explained), _expected_row(0.1, 2, sample, known, explained)]
    print(got.to_string())
    assert got.values.tolist() == want  # counts, abundance sums, and the fractions as those integers divided
    # the residual: exactly the sample hashes outside sketch(A) | sketch(B), with their abundances
    left = _check_residual(res / residual.RESIDUAL_NAME, sample, True, explained, "mix.fa residual")
    # what C shares with the sample and A and B do not hold is in the residual, and counts as "in database, unexplained"
    c_only = [h for h in sample if h in sketch[C_] and h not in explained]
    print("sample hashes held by C and not by A or B:", len(c_only), "of", len(sketch[C_]), "in C's sketch; residual:", len(left))
    assert len(c_only) >= 1 and set(c_only) <= set(left)
    row = got.iloc[0]
    assert row["num_hashes_in_database"] - row["num_hashes_explained"] == len(c_only)
    assert row["abund_in_database"] - row["abund_explained"] == sum(sample[h] for h in c_only)
    assert len([h for h in left if h in sketch[D]]) > 2000  # D is what the call set leaves
    assert sorted(os.listdir(res)) == sorted(["result.xlsx", "result_all.txt", "sheets", abundance.PROFILE_NAME,
                                              residual.EXPLAINED_NAME, residual.RESIDUAL_NAME])
    # the residual against the database that knows D: D is called present, A and B do not appear at all
    again = _run(cfg4, [res / residual.RESIDUAL_NAME], tmp_path / "again", "--residual", "--min_coverage_list", "1", "0.1")
    df4 = pd.read_csv(again / "result_all.txt", sep="\t")
    assert D in set(df4[df4["in_sample_est"]]["organism_name"]) and not ({A, B} & set(df4["organism_name"]))
    got4 = _read(again / residual.EXPLAINED_NAME)
    left_sample = {h: sample[h] for h in left}
    called = set(df4[(df4["min_coverage"] == 1.0) & df4["in_sample_est"]]["organism_name"])
    assert got4.values.tolist()[0] == _expected_row(1.0, len(called), left_sample, set().union(*sketch.values()),
                                                    set().union(*(sketch[g] for g in called)))
    # the same run without --residual lists exactly the files it lists today
    plain = _run(cfg3, [files["mix"]], tmp_path / "without", "--abundance", "--min_coverage_list", "1", "0.1")
    assert sorted(os.listdir(plain)) == sorted(["result.xlsx", "result_all.txt", "sheets", abundance.PROFILE_NAME])
    assert (plain / "result_all.txt").read_bytes() == (res / "result_all.txt").read_bytes()
    bare = _run(cfg3, [files["mix"]], tmp_path / "bare", "--min_coverage_list", "1", "0.1")
    assert sorted(os.listdir(bare)) == ["result.xlsx", "result_all.txt", "sheets"]


def test_sample_without_abundances_counts_every_hash_once(trained, tmp_path):
    tmp, cfg3, cfg4, sketch, files = trained
    res = _run(cfg3, [files["mix_flat"]], tmp_path / "flat", "--residual", "--min_coverage_list", "1", "0.1", "--residual_coverage", "1")
    sample, tracked = _sample(files["mix_flat"])
    assert not tracked and set(sample.values()) == {1}
    got = _read(res / residual.EXPLAINED_NAME)
    known, explained = sketch[A] | sketch[B] | sketch[C_], sketch[A] | sketch[B]
    assert got.values.tolist() == [_expected_row(1.0, 2, sample, known, explained), _expected_row(0.1, 2, sample, known, explained)]
    with_ab = _sample(files["mix"])[0]
    assert got["num_hashes"].tolist() == [len(with_ab)] * 2  # the same counts as the sketch with abundances ...
    for h, a in (("num_hashes", "abund_total"), ("num_hashes_in_database", "abund_in_database"), ("num_hashes_explained", "abund_explained"),
                 ("num_hashes_unexplained", "abund_unexplained"), ("f_hashes_in_database", "f_abund_in_database"),
                 ("f_hashes_explained", "f_abund_explained")):
        assert got[h].tolist() == got[a].tolist(), (h, a)  # ... and the abund columns equal the hash columns
    _check_residual(res / residual.RESIDUAL_NAME, sample, False, explained, "mix.fa residual")


def _same_files(cdir, sdir, what):
    assert (cdir / residual.EXPLAINED_NAME).read_bytes() == (sdir / residual.EXPLAINED_NAME).read_bytes(), what
    a = sigio.load_file_as_signatures(str(cdir / residual.RESIDUAL_NAME), ksize=31)
    b = sigio.load_file_as_signatures(str(sdir / residual.RESIDUAL_NAME), ksize=31)
    assert len(a) == len(b) == 1 and a[0].name == b[0].name and a[0].md5sum() == b[0].md5sum(), what
    assert np.array_equal(a[0].minhash.mins, b[0].minhash.mins) and np.array_equal(a[0].minhash.abundances, b[0].minhash.abundances), what
    assert sigio.zip_has_manifest(str(cdir / residual.RESIDUAL_NAME)), what


def test_cohort_equals_single_runs(trained, tmp_path):
    tmp, cfg3, cfg4, sketch, files = trained
    opts = ["--residual", "--min_coverage_list", "1", "0.5", "0.1", "--residual_coverage", "0.5"]
    names = ["mix", "second", "none"]
    res = _run(cfg3, [files[n] for n in names], tmp_path / "cohort", *opts)
    assert not (res / "none").exists()
    summary = _read(res / "cohort_samples.tsv").set_index("stem")
    assert list(summary.columns) == cohort.SAMPLE_COLUMNS[1:] + ["f_hashes_explained", "f_abund_explained"]
    for n in names[:2]:
        single = _run(cfg3, [files[n]], tmp_path / f"single_{n}", *opts)
        _same_files(res / n, single, n)
        assert sorted(os.listdir(res / n)) == sorted(["result.xlsx", "result_all.txt", "sheets", residual.EXPLAINED_NAME, residual.RESIDUAL_NAME])
        row = _read(single / residual.EXPLAINED_NAME)
        row = row[row["min_coverage"] == 0.5].iloc[0]
        assert summary.loc[n, "f_hashes_explained"] == row["f_hashes_explained"] > 0.1
        assert summary.loc[n, "f_abund_explained"] == row["f_abund_explained"] > 0.1
    assert summary.loc["none", "status"] == "no_overlap"
    assert summary.loc["none", "f_hashes_explained"] == 0.0 and summary.loc["none", "f_abund_explained"] == 0.0
    with pytest.raises(SystemExit):  # the single path stops at an empty multisearch result, and writes nothing new
        _run(cfg3, [files["none"]], tmp_path / "single_none", *opts)
    assert not (tmp_path / "single_none" / "results" / residual.EXPLAINED_NAME).exists()
    assert not (tmp_path / "single_none" / "results" / residual.RESIDUAL_NAME).exists()
    # the same cohort without the flag: the old columns, the old files
    plain = _run(cfg3, [files[n] for n in names], tmp_path / "cohort_plain", "--min_coverage_list", "1", "0.5", "0.1")
    assert list(pd.read_csv(plain / "cohort_samples.tsv", sep="\t").columns) == cohort.SAMPLE_COLUMNS
    for n in names[:2]:
        assert sorted(os.listdir(plain / n)) == ["result.xlsx", "result_all.txt", "sheets"]
        assert (plain / n / "result_all.txt").read_bytes() == (res / n / "result_all.txt").read_bytes()


def test_duplicate_names_in_a_cohort_equal_the_single_run(trained, tmp_path):
    """A takes B's organism name, so a sample of B pulls A's row into its tables by name (the cohort decides those on the
    host).  The call set is made of manifest ROWS: A's row is not present and explains nothing."""
    tmp, cfg3, cfg4, sketch, files = trained
    conf = json.load(open(cfg4))
    man = pd.read_csv(conf["manifest_file_path"], sep="\t")
    man.loc[man["organism_name"] == A, "organism_name"] = B
    dup_man = tmp_path / "dup_manifest.tsv"
    man.to_csv(dup_man, sep="\t", index=False)
    conf["manifest_file_path"] = str(dup_man)
    dup_cfg = tmp_path / "dup_config.json"
    dup_cfg.write_text(json.dumps(conf))
    opts = ["--residual", "--abundance", "--min_coverage_list", "1", "--show_all"]
    res = _run(dup_cfg, [files["b_twice"], files["second"]], tmp_path / "cohort", *opts)
    single = _run(dup_cfg, [files["b_twice"]], tmp_path / "single", *opts)
    _same_files(res / "b_twice", single, "duplicate names")
    df = pd.read_csv(single / "result_all.txt", sep="\t")
    assert len(df[df["organism_name"] == B]) == 2 and int(df["in_sample_est"].sum()) == 1
    sample, _ = _sample(files["b_twice"])
    got = _read(single / residual.EXPLAINED_NAME)
    assert got.values.tolist() == [_expected_row(1.0, 1, sample, set().union(*sketch.values()), sketch[B])]
    _check_residual(single / residual.RESIDUAL_NAME, sample, True, sketch[B], "b_twice.fa residual")
