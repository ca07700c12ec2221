"""`yacht run --lineages`: a per-taxon table of how many sample hashes resolve to each clade.

The device answers, per sample hash, the lowest common ancestor of its holders in a taxonomy (RefDB.lca / yh_lca) and per node
how many hashes resolve exactly there.  The taxonomy itself comes from a lineage table the user supplies -- the CSV that
sourmash's `tax` and `lca` commands take -- and everything here is plain Python / numpy / pandas on it: reading the file,
numbering the tree so that a parent comes before its children, the clade sums and the table.  No device, no library call.

A cohort (`--lineages FILE --lineages_rank RANK` with two or more sample files; yacht_amd/cohort.py) gets the same table per
sample and results/cohort_lca.tsv in long form, cut at RANK (rank_rows): over every taxon it would hold samples x taxa rows.
Hash-range shards are not built for either form.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np
import pandas as pd

from .utils import logger

RANKS = ("superkingdom", "phylum", "class", "order", "family", "genus", "species", "strain")
IDENT_COLUMNS = ("ident", "identifiers", "accession")  # (sourmash accepts the same spellings of the first column)
SUMMARY_NAME = "lca_summary.tsv"
NOT_IN_DATABASE = "not_in_database"
ROOT = "root"
SUMMARY_COLUMNS = ["rank", "lineage", "num_hashes_direct", "num_hashes_clade", "f_hashes_clade", "abund_direct", "abund_clade",
                   "f_abund_clade", "n_refs_clade"]
COHORT_NAME = "cohort_lca.tsv"
ABOVE_RANK = "above_rank"
COHORT_COLUMNS = ["sample", "lineage", "num_hashes_clade", "f_hashes_clade", "abund_clade", "f_abund_clade", "n_refs_clade"]
MSG_ONE_SAMPLE = ("--lineages takes one sample file, not {0}: a cohort's per-taxon table is cut at one rank (over every taxon it "
                  "would hold samples x taxa rows).  Add --lineages_rank RANK (one of %s), run the samples one at a time, or drop "
                  "--lineages." % ", ".join(RANKS))
MSG_RANK_WITHOUT_LINEAGES = "--lineages_rank needs --lineages."
MSG_BAD_RANK = "--lineages_rank {0} is not one of the ranks %s." % ", ".join(RANKS)
MSG_NO_FILE = "--lineages file {0} does not exist."
MSG_NO_IDENT = "--lineages file {0} has no `ident` column: its header is {1}."
MSG_DUPLICATE = "--lineages file {0} lists {1} twice with different lineages."

Lineage = Tuple[str, ...]


def read_lineages(path: str) -> Dict[str, Lineage]:
    """ident -> lineage from the CSV `ident,superkingdom,phylum,class,order,family,genus,species[,strain]`.  A lineage is the
    tuple of its rank names from the superkingdom down and ENDS AT ITS FIRST EMPTY RANK (what stands below a gap has no
    place in a tree).  Rank columns the file lacks are empty; other columns are ignored; a row without an ident is skipped.
    ValueError: a missing file, a missing `ident` column, an ident listed twice with different lineages."""
    if not os.path.isfile(path):
        raise ValueError(MSG_NO_FILE.format(path))
    out: Dict[str, Lineage] = {}
    with open(path, newline="") as f:
        reader = csv.reader(f)
        header = [h.strip() for h in next(reader, [])]
        lower = [h.lower() for h in header]
        ident_at = next((lower.index(c) for c in IDENT_COLUMNS if c in lower), None)
        if ident_at is None:
            raise ValueError(MSG_NO_IDENT.format(path, header))
        rank_at = [lower.index(r) if r in lower else None for r in RANKS]
        for row in reader:
            if len(row) <= ident_at or not row[ident_at].strip():
                continue
            ident = row[ident_at].strip()
            lineage: List[str] = []
            for at in rank_at:
                name = row[at].strip() if at is not None and at < len(row) else ""
                if not name:
                    break
                lineage.append(name)
            if out.setdefault(ident, tuple(lineage)) != tuple(lineage):
                raise ValueError(MSG_DUPLICATE.format(path, ident))
    return out


def build_tree(organism_names: Sequence[str], lineages: Dict[str, Lineage]):
    """The taxonomy RefDB.set_taxonomy takes, over the references in the order of `organism_names`.  An ident matches an
    organism whose WHOLE name, or whose first whitespace-separated token, equals it (the whole name first).  A node is a
    lineage prefix; the root is the empty one, node 0; an unmatched organism, or one whose lineage is empty, hangs at the
    root.  Nodes are numbered by (depth, lineage), so parent[v] < v, and the numbering depends on the set of lineages alone,
    not on the order of the file.  Returns (parent uint32 [n_nodes], depth uint8 [n_nodes], leaf uint32 [n_refs], node_lineages
    -- the lineage tuple of every node --, n_unmatched); the number of unmatched organisms is logged."""
    leaf_lineage: List[Lineage] = []
    n_unmatched = 0
    for name in organism_names:
        name = str(name)
        tokens = name.split()
        if name in lineages:
            leaf_lineage.append(lineages[name])
        elif tokens and tokens[0] in lineages:
            leaf_lineage.append(lineages[tokens[0]])
        else:
            leaf_lineage.append(())
            n_unmatched += 1
    prefixes = {()}
    for lin in leaf_lineage:
        for d in range(1, len(lin) + 1):
            prefixes.add(lin[:d])
    node_lineages = sorted(prefixes, key=lambda p: (len(p), p))
    index = {p: v for v, p in enumerate(node_lineages)}
    parent = np.array([index[p[:-1]] if p else 0 for p in node_lineages], dtype=np.uint32)
    depth = np.array([len(p) for p in node_lineages], dtype=np.uint8)
    leaf = np.array([index[lin] for lin in leaf_lineage], dtype=np.uint32).reshape(-1)
    if n_unmatched:
        logger.info(f"{n_unmatched} of {len(leaf_lineage)} organisms have no lineage: they hang at the root.")
    return parent, depth, leaf, node_lineages, n_unmatched


def clade_sums(parent, counts) -> np.ndarray:
    """counts [n_nodes] or [n_nodes, k] of direct assignments -> the same shape with every node's whole subtree added in.  One
    reverse sweep: parent[v] < v, so every child has been added to before its parent is."""
    parent = np.asarray(parent, dtype=np.int64)
    out = np.array(counts, dtype=np.uint64, copy=True)
    for v in range(parent.size - 1, 0, -1):
        out[parent[v]] += out[v]
    return out


def summary_frame(parent, leaf, node_lineages, counts, n_hashes: int, abund_total: int, covs: Sequence[float] = (),
                  call_sets: Sequence = ()) -> pd.DataFrame:
    """The table of lca_summary.tsv.  counts: RefDB.lca's uint64 [n_nodes, 2]; n_hashes / abund_total: the sample's size and
    the sum of its abundances (its size when the sketch has none); covs / call_sets: the user coverages and, for each, the
    manifest rows of the organisms called present (residual.call_sets_of).  First row: rank `not_in_database`, the sample
    hashes no reference holds.  Then one row per node whose clade count is non-zero, the root first, ordered by lineage.
    n_refs_clade counts the references at or under the node, n_present_min_coverage{c} those of them called present at c.
    The fractions are of the whole sample (0 for an empty one)."""
    parent = np.asarray(parent, dtype=np.int64)
    leaf = np.asarray(leaf, dtype=np.int64)
    n_nodes = parent.size
    direct = np.asarray(counts, dtype=np.uint64).reshape(n_nodes, 2)
    clade = clade_sums(parent, direct)
    refs = clade_sums(parent, np.bincount(leaf, minlength=n_nodes))
    present = [clade_sums(parent, np.bincount(leaf[np.asarray(rows, dtype=np.int64)], minlength=n_nodes)) for rows in call_sets]
    n_hashes, abund_total = int(n_hashes), int(abund_total)

    def frac(x, of):
        return int(x) / of if of else 0.0

    known_h, known_a = (int(clade[0, 0]), int(clade[0, 1])) if n_nodes else (0, 0)
    rows = [[NOT_IN_DATABASE, "", n_hashes - known_h, n_hashes - known_h, frac(n_hashes - known_h, n_hashes),
             abund_total - known_a, abund_total - known_a, frac(abund_total - known_a, abund_total), 0] + [0] * len(covs)]
    for v in sorted(range(n_nodes), key=lambda v: tuple(node_lineages[v])):
        if v != 0 and clade[v, 0] == 0:
            continue
        lin = node_lineages[v]
        rows.append([RANKS[len(lin) - 1] if lin else ROOT, ";".join(lin), int(direct[v, 0]), int(clade[v, 0]), frac(clade[v, 0], n_hashes),
                     int(direct[v, 1]), int(clade[v, 1]), frac(clade[v, 1], abund_total), int(refs[v])] + [int(p[v]) for p in present])
    return pd.DataFrame(rows, columns=SUMMARY_COLUMNS + [f"n_present_min_coverage{c}" for c in covs])


def write_summary(results_folder: str, frame: pd.DataFrame) -> str:
    """results/lca_summary.tsv.  Returns its path."""
    path = os.path.join(results_folder, SUMMARY_NAME)
    frame.to_csv(path, sep="\t", index=False)
    return path


def rank_rows(parent, leaf, node_lineages, counts, rank: str, n_hashes: int, abund_total: int) -> List[list]:
    """A sample's rows of cohort_lca.tsv behind its name, from RefDB.lca's counts [n_nodes, 2] cut at `rank`:
    [lineage, num_hashes_clade, f_hashes_clade, abund_clade, f_abund_clade, n_refs_clade].  First `not_in_database`, the
    hashes no reference holds; then `above_rank`, the hashes that resolve at a node shallower than the rank (its n_refs_clade:
    the references hung that high); then one row per taxon AT the rank whose clade count is non-zero, ordered by lineage, with
    the values of that taxon's row in lca_summary.tsv.  Every known hash resolves above the rank or under exactly one taxon
    at it, so the rows add up to the sample's hashes and abundance."""
    parent = np.asarray(parent, dtype=np.int64)
    leaf = np.asarray(leaf, dtype=np.int64)
    n_nodes = parent.size
    at = RANKS.index(rank) + 1  # a taxon's depth is the length of its lineage
    depth = np.array([len(p) for p in node_lineages], dtype=np.int64)
    direct = np.asarray(counts, dtype=np.uint64).reshape(n_nodes, 2)
    clade = clade_sums(parent, direct)
    refs = clade_sums(parent, np.bincount(leaf, minlength=n_nodes))
    n_hashes, abund_total = int(n_hashes), int(abund_total)

    def frac(x, of):
        return int(x) / of if of else 0.0

    known_h, known_a = (int(clade[0, 0]), int(clade[0, 1])) if n_nodes else (0, 0)
    above = depth < at
    above_h, above_a = int(direct[above, 0].sum(dtype=np.uint64)), int(direct[above, 1].sum(dtype=np.uint64))
    rows = [[NOT_IN_DATABASE, n_hashes - known_h, frac(n_hashes - known_h, n_hashes), abund_total - known_a,
             frac(abund_total - known_a, abund_total), 0],
            [ABOVE_RANK, above_h, frac(above_h, n_hashes), above_a, frac(above_a, abund_total), int(above[leaf].sum())]]
    for v in sorted(np.flatnonzero((depth == at) & (clade[:, 0] != 0)).tolist(), key=lambda v: tuple(node_lineages[v])):
        rows.append([";".join(node_lineages[v]), int(clade[v, 0]), frac(clade[v, 0], n_hashes), int(clade[v, 1]),
                     frac(clade[v, 1], abund_total), int(refs[v])])
    return rows


def no_overlap_rows(n_hashes: int, abund_total: int) -> List[list]:
    """rank_rows of a sample none of whose hashes the database holds: its `not_in_database` row alone."""
    n_hashes, abund_total = int(n_hashes), int(abund_total)
    return [[NOT_IN_DATABASE, n_hashes, 1.0 if n_hashes else 0.0, abund_total, 1.0 if abund_total else 0.0, 0]]


def cohort_frame(stems: Sequence[str], rows: Sequence[List[list]]) -> pd.DataFrame:
    """results/cohort_lca.tsv: the samples' rank_rows one after the other in the order given, behind a `sample` column."""
    return pd.DataFrame([[stem] + r for stem, part in zip(stems, rows) for r in part], columns=COHORT_COLUMNS)


def lineages_rank(args):
    """RANK of `--lineages_rank RANK`, the rank a cohort's table is cut at; None without the option.  ValueError when it
    comes without --lineages or names no rank."""
    rank = getattr(args, "lineages_rank", None)
    if rank is None:
        return None
    if getattr(args, "lineages", None) is None:
        raise ValueError(MSG_RANK_WITHOUT_LINEAGES)
    if str(rank) not in RANKS:
        raise ValueError(MSG_BAD_RANK.format(rank))
    return str(rank)


def lineages_option(args, n_files: int):
    """The lineage table of --lineages, read and checked, or None without the option.  ValueError for a bad or missing file,
    for --lineages_rank without --lineages or with an unknown rank, and for two or more sample files without
    --lineages_rank (the message names the option): before anything is written and before any device work.  With one sample
    file the rank is checked and otherwise ignored."""
    rank = lineages_rank(args)
    path = getattr(args, "lineages", None)
    if path is None:
        return None
    if n_files > 1 and rank is None:
        raise ValueError(MSG_ONE_SAMPLE.format(n_files))
    return read_lineages(str(path))
