"""`yacht run --lineages` without a GPU: reading the lineage table, numbering the tree, the clade sums, the summary table's
invariants, and the command line's refusals before anything is written or any device work starts."""
import json
import os
import random

import numpy as np
import pytest

from yacht_amd import cli, cohort, run_YACHT, sigio, taxonomy
from yacht_amd import hypothesis_recovery_src as hr

HEADER = "ident,superkingdom,phylum,class,order,family,genus,species,strain\n"
GOOD = HEADER + (
    "GCF_1,Bacteria,Pseudomonadota,Gamma,Entero,Enterobacteriaceae,Escherichia,Escherichia coli,K-12\n"
    "GCF_2,Bacteria,Pseudomonadota,Gamma,Entero,Enterobacteriaceae,Escherichia,Escherichia coli,\n"
    "GCF_3,Bacteria,Pseudomonadota,Gamma,Entero,Enterobacteriaceae,Salmonella,Salmonella enterica,\n"
    "GCF_4,Archaea,Euryarchaeota,,Methanobacteriales,X,Y,Z,\n"
    "whole name of an organism,Bacteria,Bacillota,,,,,,\n"
)


def _write(tmp_path, text, name="lineages.csv"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_read_lineages_good_file_and_a_gap_in_the_middle(tmp_path):
    got = taxonomy.read_lineages(_write(tmp_path, GOOD))
    assert list(got) == ["GCF_1", "GCF_2", "GCF_3", "GCF_4", "whole name of an organism"]
    assert got["GCF_1"] == ("Bacteria", "Pseudomonadota", "Gamma", "Entero", "Enterobacteriaceae", "Escherichia", "Escherichia coli", "K-12")
    assert got["GCF_2"] == got["GCF_1"][:7] and got["GCF_3"][5:] == ("Salmonella", "Salmonella enterica")
    assert got["GCF_4"] == ("Archaea", "Euryarchaeota")  # a lineage ends at its first empty rank
    assert got["whole name of an organism"] == ("Bacteria", "Bacillota")
    # no strain column, other columns in between, the same row twice: all fine
    text = "ident,taxid,superkingdom,phylum,class,order,family,genus,species\nA,562,Bacteria,P,C,O,F,G,S\nA,562,Bacteria,P,C,O,F,G,S\n"
    assert taxonomy.read_lineages(_write(tmp_path, text, "b.csv")) == {"A": ("Bacteria", "P", "C", "O", "F", "G", "S")}


def test_read_lineages_refuses(tmp_path):
    with pytest.raises(ValueError, match="does not exist"):
        taxonomy.read_lineages(str(tmp_path / "nowhere.csv"))
    with pytest.raises(ValueError, match="ident"):
        taxonomy.read_lineages(_write(tmp_path, "name,superkingdom,phylum\nA,Bacteria,P\n"))
    with pytest.raises(ValueError, match="GCF_1 twice"):
        taxonomy.read_lineages(_write(tmp_path, GOOD + "GCF_1,Bacteria,Pseudomonadota,Gamma,Entero,Enterobacteriaceae,Escherichia,Escherichia albertii,\n", "c.csv"))


NAMES = ["GCF_1 Escherichia coli str. K-12", "GCF_2", "GCF_3 Salmonella", "unknown organism", "GCF_4 an archaeon",
         "whole name of an organism", "GCF_30 not GCF_3"]


def test_build_tree_numbering_depths_and_matching(tmp_path):
    lineages = taxonomy.read_lineages(_write(tmp_path, GOOD))
    parent, depth, leaf, node_lineages, n_unmatched = taxonomy.build_tree(NAMES, lineages)
    assert parent.dtype == np.uint32 and depth.dtype == np.uint8 and leaf.dtype == np.uint32 and leaf.shape == (len(NAMES),)
    assert node_lineages[0] == () and parent[0] == 0 and depth[0] == 0
    assert all(parent[v] < v for v in range(1, parent.size))
    assert all(depth[v] == depth[parent[v]] + 1 == len(node_lineages[v]) for v in range(1, parent.size))
    assert all(node_lineages[parent[v]] == node_lineages[v][:-1] for v in range(1, parent.size))
    assert len(set(node_lineages)) == len(node_lineages) == 1 + 8 + 2 + 2 + 1  # root, E. coli's eight, Salmonella's two, Archaea's two, Bacillota
    assert int(depth.max()) == 8
    # the first token matches, the whole name matches, a longer token does not; unmatched organisms hang at the root
    assert node_lineages[leaf[0]] == lineages["GCF_1"] and node_lineages[leaf[1]] == lineages["GCF_2"]
    assert node_lineages[leaf[2]][-1] == "Salmonella enterica" and node_lineages[leaf[4]] == ("Archaea", "Euryarchaeota")
    assert node_lineages[leaf[5]] == ("Bacteria", "Bacillota")
    assert leaf[3] == 0 and leaf[6] == 0 and n_unmatched == 2
    assert parent[leaf[0]] == leaf[1]  # the strain under its species, where another reference sits


def test_build_tree_is_deterministic_under_a_shuffled_file(tmp_path):
    rows = GOOD.splitlines(keepends=True)[1:]
    want = taxonomy.build_tree(NAMES, taxonomy.read_lineages(_write(tmp_path, GOOD)))
    for seed in range(3):
        random.Random(seed).shuffle(rows)
        got = taxonomy.build_tree(NAMES, taxonomy.read_lineages(_write(tmp_path, HEADER + "".join(rows), f"s{seed}.csv")))
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3] and got[4] == want[4]


def test_clade_sums_on_a_small_tree():
    #        0
    #      1   2
    #     3 4    5
    #    6
    parent = np.array([0, 0, 0, 1, 1, 2, 3], np.uint32)
    direct = np.array([[1, 10], [2, 20], [0, 0], [4, 40], [8, 80], [16, 160], [32, 2 ** 40]], np.uint64)
    clade = taxonomy.clade_sums(parent, direct)
    assert clade.dtype == np.uint64 and clade[:, 0].tolist() == [63, 46, 16, 36, 8, 16, 32]
    assert clade[:, 1].tolist() == [310 + 2 ** 40, 140 + 2 ** 40, 160, 40 + 2 ** 40, 80, 160, 2 ** 40]
    assert direct[0].tolist() == [1, 10]  # (the input is left alone)
    assert taxonomy.clade_sums(parent, np.ones(7, np.int64)).tolist() == [7, 4, 2, 2, 1, 1, 1]
    assert taxonomy.clade_sums(np.zeros(1, np.uint32), np.array([[5, 6]], np.uint64)).tolist() == [[5, 6]]


def test_summary_frame_invariants(tmp_path):
    lineages = taxonomy.read_lineages(_write(tmp_path, GOOD))
    parent, depth, leaf, node_lineages, _ = taxonomy.build_tree(NAMES, lineages)
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 50, (parent.size, 2)).astype(np.uint64)
    counts[:, 1] += counts[:, 0]
    counts[leaf[4]] = 0  # the archaeon and everything above it: an empty clade, no row
    counts[parent[leaf[4]]] = 0
    n_hashes, abund_total = int(counts[:, 0].sum()) + 17, int(counts[:, 1].sum()) + 40
    covs, call_sets = [1.0, 0.1], [np.array([0]), np.array([0, 1, 2, 3])]
    frame = taxonomy.summary_frame(parent, leaf, node_lineages, counts, n_hashes, abund_total, covs, call_sets)
    assert list(frame.columns) == taxonomy.SUMMARY_COLUMNS + ["n_present_min_coverage1.0", "n_present_min_coverage0.1"]
    assert frame["rank"].tolist()[:3] == ["not_in_database", "root", "superkingdom"] and frame["lineage"].tolist()[:2] == ["", ""]
    assert not frame["lineage"].str.startswith("Archaea").any() and len(frame) == 1 + parent.size - 2
    body = frame.iloc[1:]
    assert body["lineage"].tolist() == sorted(body["lineage"].tolist(), key=lambda s: tuple(s.split(";")) if s else ())
    # what no reference holds plus the root's clade is the sample, in hashes and in abundance
    assert frame["num_hashes_clade"][0] + frame["num_hashes_clade"][1] == n_hashes and frame["num_hashes_direct"][0] == 17
    assert frame["abund_clade"][0] + frame["abund_clade"][1] == abund_total and frame["abund_direct"][0] == 40
    assert frame["f_hashes_clade"][0] + frame["f_hashes_clade"][1] == pytest.approx(1.0)
    by_lineage = {row.lineage: row for row in body.itertuples()}
    for lin, row in by_lineage.items():
        assert row.num_hashes_direct <= row.num_hashes_clade and row.abund_direct <= row.abund_clade
        if lin:  # a child's clade is at most its parent's
            up = by_lineage[";".join(lin.split(";")[:-1])]
            assert row.num_hashes_clade <= up.num_hashes_clade and row.abund_clade <= up.abund_clade and row.n_refs_clade <= up.n_refs_clade
    root = by_lineage[""]
    assert root.n_refs_clade == len(NAMES) and root._10 == 1 and root._11 == 4
    coli = by_lineage[";".join(lineages["GCF_2"])]
    assert coli.rank == "species" and coli.n_refs_clade == 2 and coli._10 == 1 and coli._11 == 2
    # an empty sample: the two rows that always exist, fractions 0
    empty = taxonomy.summary_frame(parent, leaf, node_lineages, np.zeros_like(counts), 0, 0)
    assert empty["rank"].tolist() == ["not_in_database", "root"] and not empty["f_hashes_clade"].any()
    path = taxonomy.write_summary(str(tmp_path), frame)
    assert os.path.basename(path) == "lca_summary.tsv" and open(path).readline().split("\t")[:3] == ["rank", "lineage", "num_hashes_direct"]


@pytest.fixture
def setup(tmp_path, monkeypatch):
    """A hand-written config + manifest, an output directory, and a guard that fails on device work (tests/test_residual_cpu.py)."""
    work = tmp_path / "db_intermediate_files"
    work.mkdir()
    manifest = tmp_path / "db_processed_manifest.tsv"
    manifest.write_text("organism_name\tmd5sum\tnum_unique_kmers_in_genome_sketch\tnum_total_kmers_in_genome_sketch\t"
                        "genome_scale_factor\norg\tabcd\t10\t10\t1000\n")
    cfg = tmp_path / "db_config.json"
    cfg.write_text(json.dumps({"manifest_file_path": str(manifest), "intermediate_files_dir": str(work), "scale": 1000,
                               "ksize": 31, "ani_thresh": 0.95}))
    out = tmp_path / "out"
    out.mkdir()

    def no_device(*a, **k):
        raise AssertionError("device work started before every input was checked")

    monkeypatch.setattr(hr, "get_reference_db", no_device)
    monkeypatch.setattr(cohort, "_Device", no_device)
    return tmp_path, cfg, out


def _sample(path, seed=0):
    rng = np.random.default_rng(seed)
    mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 200, dtype=np.uint64))
    sigio.write_sig_zip([sigio.make_signature(mins, ksize=31, scaled=1000, name=os.path.basename(str(path)))], str(path))
    return path


def test_a_bad_or_missing_lineage_file_raises_before_results_exist(setup):
    tmp, cfg, out = setup
    base = ["run", "--json", str(cfg), "--sample_file", str(_sample(tmp / "s.sig.zip")), "--outdir", str(out)]
    with pytest.raises(ValueError, match="does not exist"):
        cli.main(base + ["--lineages", str(tmp / "nowhere.csv")])
    with pytest.raises(ValueError, match="ident"):
        cli.main(base + ["--lineages", _write(tmp, "name,superkingdom\nA,Bacteria\n", "noident.csv")])
    with pytest.raises(ValueError, match="twice"):
        cli.main(base + ["--lineages", _write(tmp, HEADER + "A,Bacteria,P,,,,,,\nA,Archaea,P,,,,,,\n", "dup.csv")])
    assert not list(out.iterdir())  # no results/ yet
    # a good file passes every check and stops at the device guard
    with pytest.raises(AssertionError, match="device work"):
        cli.main(base + ["--lineages", _write(tmp, GOOD)])


def test_two_sample_files_with_lineages_are_refused(setup):
    tmp, cfg, out = setup
    files = [str(_sample(tmp / f"s{i}.sig.zip", seed=i)) for i in range(2)]
    with pytest.raises(ValueError, match="--lineages") as ei:
        cli.main(["run", "--json", str(cfg), "--sample_file", *files, "--outdir", str(out), "--lineages", _write(tmp, GOOD)])
    assert "one sample file, not 2" in str(ei.value) and not list(out.iterdir())


def test_parser_and_help_list_the_option():
    base = ["run", "--json", "c.json", "--sample_file", "a.sig.zip"]
    assert cli.build_parser().parse_args(base).lineages is None
    assert cli.build_parser().parse_args(base + ["--lineages", "x.csv"]).lineages == "x.csv"
    assert "--lineages" in [f for f, _ in run_YACHT.ARGUMENTS]
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["run", "--help"])


def test_help_text(capsys):
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["run", "--help"])
    text = capsys.readouterr().out
    assert "--lineages" in text and "lca_summary.tsv" in text
