"""`yacht run --residual`: how much of a sample the organisms called present account for, and what they leave.

The device answers one byte per sample hash (RefDB.explain / yh_explain): bit 7 = some reference of the database holds the
hash, bit k = some reference of call set k holds it, where call set k is the organisms called present at the k-th
min_coverage; and per bit the number of such hashes and the sum of their abundances.  Everything here is numpy / pandas on
those numbers: no device, no library call.
"""
from __future__ import annotations

import os
from typing import List, Sequence

import numpy as np
import pandas as pd

from . import sigio

MAX_SETS = 7  # call sets per explain call: bits 0..6 of a member byte
KNOWN_BIT = 7  # bit 7 of a flag: the hash is in the database
EXPLAINED_COLUMNS = [
    "min_coverage",
    "num_present_organisms",
    "num_hashes",
    "num_hashes_in_database",
    "num_hashes_explained",
    "num_hashes_unexplained",
    "abund_total",
    "abund_in_database",
    "abund_explained",
    "abund_unexplained",
    "f_hashes_in_database",
    "f_hashes_explained",
    "f_abund_in_database",
    "f_abund_explained",
]
EXPLAINED_NAME = "sample_explained.tsv"
RESIDUAL_NAME = "residual.sig.zip"
COHORT_COLUMNS = ["f_hashes_explained", "f_abund_explained"]  # of cohort_samples.tsv, for --residual_coverage
MSG_COVERAGE_WITHOUT_RESIDUAL = "--residual_coverage needs --residual."
MSG_COVERAGE_NOT_LISTED = "--residual_coverage {0} is not one of the --min_coverage_list values {1}."


def residual_coverage(args) -> float:
    """The coverage whose residual is written: --residual_coverage, by default the smallest of --min_coverage_list.
    ValueError when the option comes without --residual or names a value outside the list.  Host only."""
    want = bool(getattr(args, "residual", False))
    cov = getattr(args, "residual_coverage", None)
    if not want:
        if cov is not None:
            raise ValueError(MSG_COVERAGE_WITHOUT_RESIDUAL)
        return float("nan")
    listed = sorted(set(float(c) for c in args.min_coverage_list), reverse=True)
    if cov is None:
        return listed[-1]
    if float(cov) not in listed:
        raise ValueError(MSG_COVERAGE_NOT_LISTED.format(cov, listed))
    return float(cov)


def member_table(n_refs: int, call_sets: Sequence) -> np.ndarray:
    """The member table of RefDB.explain, uint8 [n_refs], from up to seven call sets (arrays of manifest row indices):
    call set k sets bit k at its rows.  ValueError for more than seven (member_tables splits them)."""
    if len(call_sets) > MAX_SETS:
        raise ValueError(f"a member table holds at most {MAX_SETS} call sets, not {len(call_sets)}")
    table = np.zeros(int(n_refs), dtype=np.uint8)
    for k, rows in enumerate(call_sets):
        rows = np.asarray(rows, dtype=np.int64)
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= int(n_refs)):
            raise ValueError(f"call set {k} names a row outside [0, {int(n_refs)})")
        table[rows] |= np.uint8(1 << k)
    return table


def member_tables(n_refs: int, call_sets: Sequence) -> List[np.ndarray]:
    """One member table per seven call sets (at least one): call set c is bit c % 7 of table c // 7."""
    return [member_table(n_refs, call_sets[i:i + MAX_SETS]) for i in range(0, max(len(call_sets), 1), MAX_SETS)]


def explain_call_sets(db, sample, abund, call_sets: Sequence):
    """RefDB.explain for any number of call sets, seven per call.  Returns (flags, totals): flags[c] uint8 [n] and
    totals[c] uint64 [8, 2] are those of the call that answered call set c, whose bit there is c % 7."""
    flags, totals = [], []
    for table in member_tables(db.n_refs, call_sets):
        f, t = db.explain(sample, table, abund)
        flags.append(f)
        totals.append(t)
    return [flags[c // MAX_SETS] for c in range(len(call_sets))], [totals[c // MAX_SETS] for c in range(len(call_sets))]


def explained_frame(covs: Sequence[float], n_present: Sequence[int], totals: Sequence, n_hashes: int, abund_total: int) -> pd.DataFrame:
    """One row per user coverage, coverage descending (EXPLAINED_COLUMNS).  covs[c] / n_present[c]: the c-th coverage and
    the number of organisms called present at it; totals: one uint64 [8, 2] array for all coverages (at most seven), or
    one per coverage, call set c being bit c % 7 of totals[c]; n_hashes / abund_total: the size of the sample and the sum
    of its abundances (its size when the sketch has none).  unexplained = total - explained; the fractions are 0 for an
    empty sample."""
    if isinstance(totals, np.ndarray) and totals.ndim == 2:
        totals = [totals] * len(covs)
    n_hashes, abund_total = int(n_hashes), int(abund_total)
    rows = []
    for c, (cov, present) in enumerate(zip(covs, n_present)):
        t = np.asarray(totals[c], dtype=np.uint64).reshape(8, 2)
        bit = c % MAX_SETS
        h_db, a_db = int(t[KNOWN_BIT, 0]), int(t[KNOWN_BIT, 1])
        h_ex, a_ex = int(t[bit, 0]), int(t[bit, 1])
        rows.append((float(cov), int(present), n_hashes, h_db, h_ex, n_hashes - h_ex, abund_total, a_db, a_ex, abund_total - a_ex,
                     h_db / n_hashes if n_hashes else 0.0, h_ex / n_hashes if n_hashes else 0.0,
                     a_db / abund_total if abund_total else 0.0, a_ex / abund_total if abund_total else 0.0))
    rows.sort(key=lambda r: -r[0])
    return pd.DataFrame(rows, columns=EXPLAINED_COLUMNS)


def residual_signature(sample_sig, flags, bit: int, coverage: float):
    """The sample's signature restricted to the hashes whose flag has `bit` clear: what the call set of `coverage` does
    not explain.  Hashes stay ascending, abundances are kept exactly when the sample tracks them, ksize, scaled and seed
    are unchanged, and the name is "<sample name> residual"."""
    mh = sample_sig.minhash
    flags = np.asarray(flags, dtype=np.uint8)
    if flags.size != len(mh):
        raise ValueError(f"{flags.size} flags for {len(mh)} sample hashes")
    keep = (flags & np.uint8(1 << int(bit))) == 0
    mins = np.asarray(mh.mins, dtype=np.uint64)[keep]
    ab = None if mh.abundances is None else np.asarray(mh.abundances)[keep]
    out = sigio.MinHash(mins, mh.ksize, mh.max_hash, ab, seed=mh.seed, molecule="dna" if mh.moltype == "DNA" else mh.moltype, num=mh.num)
    return sigio.Signature(out, f"{sample_sig.name} residual", getattr(sample_sig, "filename", ""))


def sample_abundances_or_none(sample_sig):
    """The per-hash abundances of a sample's sketch in the order of its hashes, or None when the sketch tracks none."""
    mh = sample_sig.minhash
    return None if mh.abundances is None else np.asarray(mh.abundances)


def call_sets_of(manifest_names, tables: Sequence[pd.DataFrame]) -> List[np.ndarray]:
    """Per coverage table (hypothesis_recovery's, before or after trimming), the manifest rows of the organisms it calls
    present.  A table holds the manifest rows whose organism name it lists, in manifest order, so its i-th row is the i-th
    of np.flatnonzero(names.isin(listed)): the mapping the abundance path uses, exact with duplicate organism names too."""
    names = pd.Series(np.asarray(manifest_names))
    out = []
    for df in tables:
        rows = np.flatnonzero(names.isin(df["organism_name"]).to_numpy())
        if rows.size != len(df):
            raise ValueError(f"a result table of {len(df)} rows selects {rows.size} manifest rows")
        out.append(rows[df["in_sample_est"].to_numpy().astype(bool)])
    return out


def write_outputs(results_folder: str, sample_sig, covs: Sequence[float], call_sets: Sequence, flags: Sequence, totals: Sequence,
                  coverage: float) -> pd.DataFrame:
    """results/sample_explained.tsv over the user coverages and results/residual.sig.zip for `coverage`.  covs, call_sets,
    flags and totals run in parallel (explain_call_sets).  Returns the frame."""
    mh = sample_sig.minhash
    n_hashes = len(mh)
    abund_total = n_hashes if mh.abundances is None else int(np.asarray(mh.abundances, dtype=np.uint64).sum(dtype=np.uint64))
    frame = explained_frame(covs, [len(s) for s in call_sets], totals, n_hashes, abund_total)
    frame.to_csv(os.path.join(results_folder, EXPLAINED_NAME), sep="\t", index=False)
    c = [float(x) for x in covs].index(float(coverage))
    sigio.write_sig_zip([residual_signature(sample_sig, flags[c], c % MAX_SETS, coverage)], os.path.join(results_folder, RESIDUAL_NAME))
    return frame
