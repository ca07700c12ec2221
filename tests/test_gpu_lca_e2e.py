"""`yacht run --lineages` from sequence to lca_summary.tsv, on the GPU.

The database is `yacht sketch ref` + `yacht train` over the four GCF_*_genomic.fna.gz fixtures (unrelated genomes) plus a
fifth genome the test writes, a chimera: a tenth of genome A's bases, a tenth of genome B's, the rest seeded random bases.  Its
containment in A and in B stays near 0.1, below 0.95^31 = 0.2039, so training keeps all five.  The lineage file puts the
chimera in A's genus and in another phylum than B, C in A's family, and leaves D without a lineage: hashes A shares with the
chimera resolve to their genus, hashes B shares with it to the superkingdom.  The sample holds A three times, B once, D twice
and a sliver of C.  Every expected number comes from Python sets over the five reference sketches and the sample sketch, with
the LCA taken as the common prefix of the holders' lineages."""
import gzip
import json
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from yacht_amd import cli, residual, sigio, taxonomy

pytestmark = pytest.mark.gpu

FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")
GENOMES = ["GCF_018918045.1_genomic", "GCF_018918095.1_genomic", "GCF_018918185.1_genomic", "GCF_018918235.1_genomic"]
A, B, C_, D = GENOMES[0], GENOMES[3], GENOMES[1], GENOMES[2]
CHIMERA = "CHIMERA_1.1_genomic"
SLIVER = 12_000  # bases of C's first record in the sample
FAMILY = ("Bacteria", "P1", "C1", "O1", "F1")
LINEAGE = {A: FAMILY + ("G1", "G1 a"), CHIMERA: FAMILY + ("G1", "G1 chimaera"), C_: FAMILY + ("G2", "G2 c"),
           B: ("Bacteria", "P2", "C2", "O2", "F2", "G3", "G3 b")}  # (D has none)


def _text(genome):
    with gzip.open(os.path.join(FX, genome + ".fna.gz"), "rb") as f:
        text = f.read()
    return text if text.endswith(b"\n") else text + b"\n"


def _bases(genome):
    return b"".join(line for line in _text(genome).split(b"\n") if not line.startswith(b">"))


def _write_chimera(path):
    a, b = _bases(A), _bases(B)
    rng = np.random.default_rng(77)
    rest = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(a) - len(a) // 10 - len(b) // 10)].tobytes()
    with gzip.open(path, "wb", compresslevel=1) as f:
        for name, seq in (("from_a", a[:len(a) // 10]), ("from_b", b[:len(b) // 10]), ("random", rest)):
            f.write(b">" + name.encode() + b"\n")
            f.write(b"\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + b"\n")


@pytest.fixture(scope="module")
def trained(hip_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lca_e2e")
    gdir = tmp / "genomes"
    gdir.mkdir()
    for g in GENOMES:
        shutil.copyfile(os.path.join(FX, g + ".fna.gz"), gdir / (g + ".fna.gz"))
    _write_chimera(gdir / (CHIMERA + ".fna.gz"))
    ref_zip = tmp / "refs.sig.zip"
    cli.main(["sketch", "ref", "--infile", str(gdir), "--kmer", "31", "--scaled", "1000", "--outfile", str(ref_zip)])
    out = tmp / "db5"
    out.mkdir()
    assert cli.main(["train", "--ref_file", str(ref_zip), "--ksize", "31", "--prefix", "db5", "--ani_thresh", "0.95",
                     "--outdir", str(out), "--num_threads", "2", "--force"]) == 0
    cfg = out / "db5_config.json"
    man = pd.read_csv(json.load(open(cfg))["manifest_file_path"], sep="\t")
    assert sorted(man["organism_name"]) == sorted(GENOMES + [CHIMERA])  # training kept all five
    sketch = {s.name: set(int(h) for h in s.minhash.mins) for s in sigio.load_file_as_signatures(str(ref_zip), ksize=31)}
    assert sorted(sketch) == sorted(GENOMES + [CHIMERA])
    for g in (A, B):  # the chimera's containment in either parent stays below 0.95^31
        share = len(sketch[CHIMERA] & sketch[g])
        print("chimera shares", share, "of", len(sketch[CHIMERA]), "hashes with", g)
        assert 50 < share < 0.2039 * len(sketch[CHIMERA])
    fasta = tmp / "mix.fa"
    with open(fasta, "wb") as f:
        f.write(_text(A) * 3 + _text(B) + _text(D) * 2 + b">sliver\n" + _bases(C_)[:SLIVER] + b"\n")
    sample = tmp / "mix.sig.zip"
    cli.main(["sketch", "sample", "--infile", str(fasta), "--kmer", "31", "--scaled", "1000", "--outfile", str(sample)])
    lineages = tmp / "lineages.csv"
    with open(lineages, "w") as f:
        f.write("ident," + ",".join(taxonomy.RANKS) + "\n")
        for g, lin in LINEAGE.items():
            f.write(",".join([g] + list(lin) + [""] * (len(taxonomy.RANKS) - len(lin))) + "\n")
    return tmp, cfg, sketch, sample, lineages


def _run(cfg, sample, outdir, *opts):
    outdir.mkdir()
    assert cli.main(["run", "--json", str(cfg), "--sample_file", str(sample), "--num_threads", "2", "--outdir", str(outdir), *opts]) == 0
    return outdir / "results"


def _expected(sketch, sample, covs, present):
    """The rows of lca_summary.tsv from Python sets.  sample: {hash: abundance}; present[c]: the organisms called at covs[c]."""
    lineage = {g: LINEAGE.get(g, ()) for g in sketch}
    n, total = len(sample), sum(sample.values())
    direct = {}
    for h, a in sample.items():
        holders = [lineage[g] for g in sketch if h in sketch[g]]
        if not holders:
            continue
        common = holders[0]
        for lin in holders[1:]:
            k = 0
            while k < min(len(common), len(lin)) and common[k] == lin[k]:
                k += 1
            common = common[:k]
        d = direct.setdefault(common, [0, 0])
        d[0] += 1
        d[1] += a
    prefixes = sorted({lin[:k] for lin in lineage.values() for k in range(len(lin) + 1)})
    known = [sum(d[0] for d in direct.values()), sum(d[1] for d in direct.values())]
    rows = [["not_in_database", np.nan, n - known[0], n - known[0], (n - known[0]) / n, total - known[1], total - known[1],
             (total - known[1]) / total, 0] + [0] * len(covs)]
    for p in prefixes:
        under = [lin for lin in direct if lin[:len(p)] == p]
        clade = [sum(direct[lin][0] for lin in under), sum(direct[lin][1] for lin in under)]
        if p and clade[0] == 0:
            continue
        mine = direct.get(p, [0, 0])
        rows.append([taxonomy.RANKS[len(p) - 1] if p else "root", ";".join(p) if p else np.nan, mine[0], clade[0], clade[0] / n, mine[1], clade[1],
                     clade[1] / total, sum(1 for g in lineage if lineage[g][:len(p)] == p)]
                    + [sum(1 for g in called if lineage[g][:len(p)] == p) for called in present])
    return rows


def test_lca_summary_of_a_mix_from_sequence(trained, tmp_path):
    tmp, cfg, sketch, sample_file, lineages = trained
    covs = ["1", "0.1"]
    res = _run(cfg, sample_file, tmp_path / "with", "--lineages", str(lineages), "--residual", "--abundance", "--min_coverage_list", *covs)
    df = pd.read_csv(res / "result_all.txt", sep="\t")
    present = [set(df[(df["min_coverage"] == float(c)) & df["in_sample_est"]]["organism_name"]) for c in covs]
    assert present[0] >= {A, B, D} and CHIMERA not in present[0]
    mh = sigio.load_file_as_signatures(str(sample_file), ksize=31)[0].minhash
    assert mh.abundances is not None
    sample = {int(h): int(a) for h, a in zip(mh.mins, mh.abundances)}
    got = pd.read_csv(res / taxonomy.SUMMARY_NAME, sep="\t", float_precision="round_trip")
    print(got.to_string())
    assert list(got.columns) == taxonomy.SUMMARY_COLUMNS + ["n_present_min_coverage1.0", "n_present_min_coverage0.1"]
    want = pd.DataFrame(_expected(sketch, sample, covs, present), columns=got.columns)
    assert got["rank"].tolist()[:3] == ["not_in_database", "root", "superkingdom"]
    assert got.fillna("").values.tolist() == want.fillna("").values.tolist()  # row for row: counts, sums, and the fractions as those integers divided
    by = got.fillna("").set_index("lineage")
    genus = by.loc[";".join(FAMILY + ("G1",))]
    assert genus["rank"] == "genus" and genus["num_hashes_direct"] > 50  # what A shares with the chimera
    assert genus["n_refs_clade"] == 2 and genus["n_present_min_coverage1.0"] == 1  # A is called, the chimera is not
    assert by.loc["Bacteria", "num_hashes_direct"] > 50  # what B shares with the chimera: two phyla
    root = got[got["rank"] == "root"].iloc[0]
    assert root["num_hashes_direct"] >= len(sketch[D] & set(sample)) > 2000  # D has no lineage: its hashes stay at the root
    assert root["n_refs_clade"] == 5 and root["n_present_min_coverage1.0"] == len(present[0])
    assert got["num_hashes_clade"][0] + got["num_hashes_clade"][1] == len(sample)
    # it combines with the other options: their files are there, and the explained total is the root's clade
    explained = pd.read_csv(res / residual.EXPLAINED_NAME, sep="\t")
    assert explained["num_hashes_in_database"].tolist() == [got["num_hashes_clade"][1]] * 2
    assert explained["abund_in_database"].tolist() == [got["abund_clade"][1]] * 2
    # the same run without --lineages writes the same files, byte for byte, and no lca_summary.tsv
    # (result.xlsx is a zip archive that carries the time it was written: its sheets are compared as sheets/*.tsv)
    plain = _run(cfg, sample_file, tmp_path / "without", "--residual", "--abundance", "--min_coverage_list", *covs)
    assert sorted(os.listdir(plain)) == sorted(set(os.listdir(res)) - {taxonomy.SUMMARY_NAME}) and taxonomy.SUMMARY_NAME in os.listdir(res)
    for name in ["result_all.txt", residual.EXPLAINED_NAME, "abundance_profile.tsv"] + [os.path.join("sheets", s) for s in sorted(os.listdir(res / "sheets"))]:
        assert (plain / name).read_bytes() == (res / name).read_bytes(), name
    assert sorted(os.listdir(plain / "sheets")) == sorted(os.listdir(res / "sheets"))


def test_sample_without_abundances_and_with_gather(trained, tmp_path):
    """A sketch that tracks no abundances: the abund columns equal the hash columns; --gather runs beside it."""
    tmp, cfg, sketch, sample_file, lineages = trained
    mix = sigio.load_file_as_signatures(str(sample_file), ksize=31)[0]
    flat = tmp_path / "mix_flat.sig.zip"
    sigio.write_sig_zip([sigio.make_signature(mix.minhash.mins, ksize=31, scaled=1000, name=mix.name)], str(flat))
    res = _run(cfg, flat, tmp_path / "flat", "--lineages", str(lineages), "--gather", "--min_coverage_list", "1")
    df = pd.read_csv(res / "result_all.txt", sep="\t")
    present = [set(df[(df["min_coverage"] == 1.0) & df["in_sample_est"]]["organism_name"])]
    got = pd.read_csv(res / taxonomy.SUMMARY_NAME, sep="\t", float_precision="round_trip")
    want = pd.DataFrame(_expected(sketch, {int(h): 1 for h in mix.minhash.mins}, ["1"], present), columns=got.columns)
    assert got.fillna("").values.tolist() == want.fillna("").values.tolist()
    for h, a in (("num_hashes_direct", "abund_direct"), ("num_hashes_clade", "abund_clade"), ("f_hashes_clade", "f_abund_clade")):
        assert got[h].tolist() == got[a].tolist(), (h, a)
    assert "gather_profile.tsv" in os.listdir(res)
