"""`yacht classify` from sequence to classify_records.tsv and classify_summary.tsv, on the GPU.

The database, the chimera and the lineage file are those of test_gpu_lca_e2e.py, restated: the four GCF_*_genomic.fna.gz
fixtures plus a chimera (a tenth of A, a tenth of B, the rest random) in A's genus; C in A's family; B in another phylum; D
without a lineage.  The FASTA to classify holds A's and B's contigs, 5 kb pieces of the chimera's three parts, D's contigs
(no lineage: uninformative), seeded random records (not in the database) and a 20-base record (no hashes).  Every expected
status and lineage comes from Python sets over the five reference sketches and sketch_sequences of each record, with the LCA
taken as the common prefix of lineages.  The two files are then byte-identical for a small chunk budget, the default budget and
the YACHT_CLASSIFY=loop route, each run in its own process."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from yacht_amd import classify, cli, sigio, sketch, taxonomy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")
GENOMES = ["GCF_018918045.1_genomic", "GCF_018918095.1_genomic", "GCF_018918185.1_genomic", "GCF_018918235.1_genomic"]
A, B, C_, D = GENOMES[0], GENOMES[3], GENOMES[1], GENOMES[2]
CHIMERA = "CHIMERA_1.1_genomic"
FAMILY = ("Bacteria", "P1", "C1", "O1", "F1")
LINEAGE = {A: FAMILY + ("G1", "G1 a"), CHIMERA: FAMILY + ("G1", "G1 chimaera"), C_: FAMILY + ("G2", "G2 c"),
           B: ("Bacteria", "P2", "C2", "O2", "F2", "G3", "G3 b")}  # (D has none)
MIN_HITS = 2


def _records_of(genome):
    with gzip.open(os.path.join(FX, genome + ".fna.gz"), "rb") as f:
        text = f.read()
    recs, name, parts = [], None, []
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            if name is not None:
                recs.append((name, b"".join(parts)))
            name, parts = line[1:].decode(), []
        elif line.strip():
            parts.append(line.strip())
    if name is not None:
        recs.append((name, b"".join(parts)))
    return recs


def _bases(genome):
    return b"".join(s for _n, s in _records_of(genome))


def _chimera_parts():
    a, b = _bases(A), _bases(B)
    rng = np.random.default_rng(77)
    rest = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(a) - len(a) // 10 - len(b) // 10)].tobytes()
    return (("from_a", a[:len(a) // 10]), ("from_b", b[:len(b) // 10]), ("random", rest))


def _write_fasta(path, records, gz=False):
    opener = (lambda p: gzip.open(p, "wb", compresslevel=1)) if gz else (lambda p: open(p, "wb"))
    with opener(path) as f:
        for name, seq in records:
            f.write(b">" + name.encode() + b"\n")
            f.write(b"\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + b"\n")


def _common(lins):
    common = lins[0]
    for lin in lins[1:]:
        k = 0
        while k < min(len(common), len(lin)) and common[k] == lin[k]:
            k += 1
        common = common[:k]
    return common


@pytest.fixture(scope="module")
def trained(hip_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("classify_e2e")
    gdir = tmp / "genomes"
    gdir.mkdir()
    for g in GENOMES:
        shutil.copyfile(os.path.join(FX, g + ".fna.gz"), gdir / (g + ".fna.gz"))
    parts = _chimera_parts()
    _write_fasta(gdir / (CHIMERA + ".fna.gz"), parts, gz=True)
    ref_zip = tmp / "refs.sig.zip"
    cli.main(["sketch", "ref", "--infile", str(gdir), "--kmer", "31", "--scaled", "1000", "--outfile", str(ref_zip)])
    out = tmp / "db5"
    out.mkdir()
    assert cli.main(["train", "--ref_file", str(ref_zip), "--ksize", "31", "--prefix", "db5", "--ani_thresh", "0.95",
                     "--outdir", str(out), "--num_threads", "2", "--force"]) == 0
    cfg = out / "db5_config.json"
    man = pd.read_csv(json.load(open(cfg))["manifest_file_path"], sep="\t")
    assert sorted(man["organism_name"]) == sorted(GENOMES + [CHIMERA])  # training kept all five
    ref = {s.name: set(int(h) for h in s.minhash.mins) for s in sigio.load_file_as_signatures(str(ref_zip), ksize=31)}
    lineages = tmp / "lineages.csv"
    with open(lineages, "w") as f:
        f.write("ident," + ",".join(taxonomy.RANKS) + "\n")
        for g, lin in LINEAGE.items():
            f.write(",".join([g] + list(lin) + [""] * (len(taxonomy.RANKS) - len(lin))) + "\n")
    rng = np.random.default_rng(5)
    records = [(n + " of A", s) for n, s in _records_of(A)] + [(n + " of B", s) for n, s in _records_of(B)]
    for name, seq in parts:
        records += [(f"chimera_{name}_{i}", seq[i:i + 5000]) for i in range(0, min(len(seq), 40_000), 5000)]
    records += [(n + " of D", s) for n, s in _records_of(D)]
    records += [(f"noise_{i} random bases", np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 6000)].tobytes()) for i in range(4)]
    records.append(("tiny", b"ACGTACGTACGTACGTACGT"))
    fasta = tmp / "contigs.fa"
    _write_fasta(fasta, records)
    return tmp, cfg, ref, lineages, fasta, records


def _expected(ref, records):
    lineage = {g: LINEAGE.get(g, ()) for g in ref}
    rows = []
    for name, seq in records:
        mins = sketch.sketch_sequences([seq], 31, 1000)[0]
        hit_lins = []
        for h in mins.tolist():
            holders = [lineage[g] for g in ref if h in ref[g]]
            if holders:
                hit_lins.append(_common(holders))
        inf = [lin for lin in hit_lins if lin]
        if len(mins) == 0:
            status = "no_hashes"
        elif not hit_lins:
            status = "not_in_database"
        elif not inf:
            status = "uninformative"
        elif len(inf) < MIN_HITS:
            status = "below_min_hits"
        else:
            status = "classified" if _common(inf) else "conflict"
        lin = _common(inf) if status == "classified" else ()
        rows.append(["contigs", name.split()[0], len(seq), len(mins), len(hit_lins), len(hit_lins) - len(inf), status,
                     taxonomy.RANKS[len(lin) - 1] if lin else "", ";".join(lin)])
    return rows


def _classify(cfg, lineages, fasta, outdir, env):
    e = dict(os.environ)
    e.pop("YACHT_CLASSIFY", None)
    e.pop("YACHT_SKETCH_BATCH_BYTES", None)
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([ROOT] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, "-m", "yacht_amd", "classify", "--json", str(cfg), "--lineages", str(lineages), "--infile", str(fasta),
                        "--outdir", str(outdir), "--num_threads", "2"], env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = outdir / "results"
    return (res / classify.RECORDS_NAME).read_bytes(), (res / classify.SUMMARY_NAME).read_bytes(), p.stdout + p.stderr


def test_classify_a_fasta_of_contigs(trained, tmp_path):
    tmp, cfg, ref, lineages, fasta, records = trained
    want = _expected(ref, records)
    statuses = [r[6] for r in want]
    print({s: statuses.count(s) for s in classify.STATUSES})
    assert {"no_hashes", "not_in_database", "uninformative", "classified"} <= set(statuses)
    by_name = {r[1]: r for r in want}
    assert by_name["tiny"][6] == "no_hashes" and all(by_name[f"noise_{i}"][6] == "not_in_database" for i in range(4))
    for part, lin in (("from_a", FAMILY + ("G1",)),      # A's bases inside the chimera: their genus
                      ("from_b", ("Bacteria",)),         # B's: two phyla, the superkingdom
                      ("random", LINEAGE[CHIMERA])):     # its own bases: the chimera's species
        got_lins = {r[8] for r in want if r[1].startswith("chimera_" + part) and r[6] == "classified"}
        assert got_lins == {";".join(lin)}, (part, got_lins)
    rec_small, sum_small, err = _classify(cfg, lineages, fasta, tmp_path / "small", {"YACHT_SKETCH_BATCH_BYTES": "4096"})
    assert "chunks" in err
    got = pd.read_csv(tmp_path / "small" / "results" / classify.RECORDS_NAME, sep="\t", keep_default_na=False)
    assert list(got.columns) == classify.RECORD_COLUMNS
    assert got.values.tolist() == want
    # the summary: status rows, then taxa; status rows + the root's clade = the input
    lines = sum_small.decode().split("\n")
    assert lines[0] == "\t".join(classify.STATUS_COLUMNS) and lines[6] == "\t".join(classify.SUMMARY_COLUMNS)
    stat = {ln.split("\t")[0]: [int(x) for x in ln.split("\t")[1:]] for ln in lines[1:6]}
    taxa = [ln.split("\t") for ln in lines[7:] if ln]
    assert taxa[0][0] == "root" and taxa[1][:2] == ["superkingdom", "Bacteria"]
    assert sum(v[0] for v in stat.values()) + int(taxa[0][3]) == len(records)
    assert sum(v[1] for v in stat.values()) + int(taxa[0][5]) == sum(len(s) for _n, s in records)
    for s in ("no_hashes", "not_in_database", "uninformative", "below_min_hits", "conflict"):
        assert stat[s] == [statuses.count(s), sum(r[2] for r in want if r[6] == s)], s
    direct = {}
    for r in want:
        if r[6] == "classified":
            direct[r[8]] = direct.get(r[8], 0) + 1
    assert {t[1]: int(t[2]) for t in taxa if int(t[2])} == direct
    # byte-identical under the default budget and by the loop route
    rec_default, sum_default, _ = _classify(cfg, lineages, fasta, tmp_path / "default", {})
    assert rec_default == rec_small and sum_default == sum_small
    rec_loop, sum_loop, err_loop = _classify(cfg, lineages, fasta, tmp_path / "loop", {"YACHT_CLASSIFY": "loop"})
    assert "loop route" in err_loop
    assert rec_loop == rec_small and sum_loop == sum_small
