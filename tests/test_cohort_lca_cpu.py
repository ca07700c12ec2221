"""`yacht run --lineages --lineages_rank RANK` over a cohort, without a GPU: the option's checks before anything is written
or any device work starts, the help text, and the rank cut of a hand-made counts array (taxonomy.rank_rows) against the
sample's own lca_summary.tsv table."""
import numpy as np
import pytest
from test_taxonomy_cpu import GOOD, NAMES, _sample, _write, setup  # noqa: F401  (the fixture: config, manifest, a device guard)

from yacht_amd import cli, run_YACHT, taxonomy


def _base(cfg, out, files):
    return ["run", "--json", str(cfg), "--sample_file", *files, "--outdir", str(out)]


def test_the_option_is_checked_before_device_work(setup):  # noqa: F811
    tmp, cfg, out = setup
    files = [str(_sample(tmp / f"s{i}.sig.zip", seed=i)) for i in range(3)]
    good = _write(tmp, GOOD)
    # a cohort without the rank stays refused, in the same words, and the message now names the way out
    with pytest.raises(ValueError, match="--lineages takes one sample file, not 3") as ei:
        cli.main(_base(cfg, out, files) + ["--lineages", good])
    assert "--lineages_rank" in str(ei.value) and all(r in str(ei.value) for r in taxonomy.RANKS)
    # the rank without the table, and a rank that is none: for one file as for several
    for some in (files[:1], files):
        with pytest.raises(ValueError, match="--lineages_rank needs --lineages"):
            cli.main(_base(cfg, out, some) + ["--lineages_rank", "genus"])
        with pytest.raises(ValueError, match="kingdom is not one of the ranks"):
            cli.main(_base(cfg, out, some) + ["--lineages", good, "--lineages_rank", "kingdom"])
    # a bad table is still refused with the rank given
    with pytest.raises(ValueError, match="does not exist"):
        cli.main(_base(cfg, out, files) + ["--lineages", str(tmp / "nowhere.csv"), "--lineages_rank", "genus"])
    assert not list(out.iterdir())  # no results/ yet
    # good options pass every check and stop at the device guard: the cohort, and one file, where the rank is ignored
    for some in (files, files[:1]):
        with pytest.raises(AssertionError, match="device work"):
            cli.main(_base(cfg, out, some) + ["--lineages", good, "--lineages_rank", "species"])


def test_parser_and_help_list_the_option(capsys):
    base = ["run", "--json", "c.json", "--sample_file", "a.sig.zip", "b.sig.zip"]
    assert cli.build_parser().parse_args(base).lineages_rank is None
    assert cli.build_parser().parse_args(base + ["--lineages", "x.csv", "--lineages_rank", "family"]).lineages_rank == "family"
    assert "--lineages_rank" in [f for f, _ in run_YACHT.ARGUMENTS]
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["run", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lineages_rank" in text and "cohort_lca.tsv" in text and all(r in text for r in taxonomy.RANKS)


def _tree(tmp_path):
    return taxonomy.build_tree(NAMES, taxonomy.read_lineages(_write(tmp_path, GOOD)))


@pytest.mark.parametrize("rank", ["superkingdom", "phylum", "genus", "species", "strain"])
def test_rank_cut_of_a_hand_made_counts_array(tmp_path, rank):
    parent, depth, leaf, node_lineages, _ = _tree(tmp_path)
    rng = np.random.default_rng(11)
    counts = rng.integers(1, 50, (parent.size, 2)).astype(np.uint64)
    counts[:, 1] += counts[:, 0]
    counts[leaf[4]] = 0  # the archaeon and everything above it: an empty clade, no row at any rank
    counts[parent[leaf[4]]] = 0
    n_hashes, abund_total = int(counts[:, 0].sum()) + 17, int(counts[:, 1].sum()) + 40
    rows = taxonomy.rank_rows(parent, leaf, node_lineages, counts, rank, n_hashes, abund_total)
    at = taxonomy.RANKS.index(rank) + 1
    assert [r[0] for r in rows[:2]] == [taxonomy.NOT_IN_DATABASE, taxonomy.ABOVE_RANK] and all(len(r) == 6 for r in rows)
    assert rows[0][1:] == [17, 17 / n_hashes, 40, 40 / abund_total, 0]
    # above the rank: the direct counts of the shallower nodes, spelled out
    shallow = [v for v in range(parent.size) if depth[v] < at]
    assert rows[1][1] == sum(int(counts[v, 0]) for v in shallow) and rows[1][3] == sum(int(counts[v, 1]) for v in shallow)
    assert rows[1][5] == sum(1 for j in range(len(NAMES)) if depth[leaf[j]] < at)
    # the taxa at the rank: ordered by lineage, none empty, none of the archaeon's, and their values are lca_summary.tsv's
    taxa = rows[2:]
    lineages = [r[0] for r in taxa]
    assert lineages == sorted(lineages, key=lambda s: tuple(s.split(";"))) and all(len(s.split(";")) == at for s in lineages)
    assert not any(s.startswith("Archaea") for s in lineages)
    frame = taxonomy.summary_frame(parent, leaf, node_lineages, counts, n_hashes, abund_total)
    want = frame[frame["rank"] == rank]
    assert lineages == want["lineage"].tolist() and len(taxa) >= 1
    for r, w in zip(taxa, want.itertuples()):
        assert r[1:] == [w.num_hashes_clade, w.f_hashes_clade, w.abund_clade, w.f_abund_clade, w.n_refs_clade]
    # the three kinds of rows add up to the sample
    assert sum(r[1] for r in rows) == n_hashes and sum(r[3] for r in rows) == abund_total


def test_rows_of_a_sample_without_overlap_and_the_long_form(tmp_path):
    parent, depth, leaf, node_lineages, _ = _tree(tmp_path)
    zero = np.zeros((parent.size, 2), np.uint64)
    # the cut of all-zero counts: nothing above the rank, no taxon
    rows = taxonomy.rank_rows(parent, leaf, node_lineages, zero, "genus", 30, 90)
    assert [r[:2] for r in rows] == [[taxonomy.NOT_IN_DATABASE, 30], [taxonomy.ABOVE_RANK, 0]]
    assert taxonomy.no_overlap_rows(30, 90) == [[taxonomy.NOT_IN_DATABASE, 30, 1.0, 90, 1.0, 0]]
    assert taxonomy.no_overlap_rows(0, 0) == [[taxonomy.NOT_IN_DATABASE, 0, 0.0, 0, 0.0, 0]]
    frame = taxonomy.cohort_frame(["a", "b"], [rows, taxonomy.no_overlap_rows(5, 5)])
    assert list(frame.columns) == taxonomy.COHORT_COLUMNS == ["sample", "lineage", "num_hashes_clade", "f_hashes_clade", "abund_clade",
                                                              "f_abund_clade", "n_refs_clade"]
    assert frame["sample"].tolist() == ["a", "a", "b"] and frame["lineage"].tolist() == ["not_in_database", "above_rank", "not_in_database"]
    assert list(taxonomy.cohort_frame([], []).columns) == taxonomy.COHORT_COLUMNS
