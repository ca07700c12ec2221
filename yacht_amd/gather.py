"""`yacht run --gather`: the organisms called present, ranked by the sample hashes each adds.

`yacht run` judges every organism on its own, and --residual says what a call set explains as a whole.  This divides the
explained part among the called organisms, a `sourmash gather` style minimum set cover: the device (RefDB.gather /
yh_gather) picks, round after round, the called organism that holds the most sample hashes nobody took yet, and credits it
with exactly those.  Everything here is numpy / pandas on its rows: no device, no library call.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np
import pandas as pd

from . import _lib

GATHER_COLUMNS = [
    "min_coverage",
    "rank",
    "organism_name",
    "num_overlap",
    "num_unique",
    "f_overlap_of_sample",
    "f_unique_of_sample",
    "abund_sum_unique",
    "mean_abund_unique",
    "f_unique_weighted",
]
GATHER_NAME = "gather_profile.tsv"
COHORT_GATHER_NAME = "cohort_gather.tsv"
TOP_MAX_COHORT = _lib.YH_GATHER_BATCH_MAX_ROWS  # a block's rounds are enqueued without a host sync: the cap bounds them
MSG_OPTION_WITHOUT_GATHER = "{0} needs --gather."
MSG_COVERAGE_NOT_LISTED = "--gather_coverage {0} is not one of the --min_coverage_list values {1}."
MSG_BAD_MIN_HITS = "--gather_min_hits must be at least 1, not {0}."
MSG_BAD_TOP = "--gather_top must be at least 1, not {0}."
MSG_TOP_ABOVE_MAX = "--gather_top must be at most {1} for a cohort, not {0}: a block's rounds are queued on the device up to that bound."
MSG_COHORT = ("--gather takes one sample file, not {0}: a cohort's samples are ranked a block at a time on the device, which "
              "needs a bound on the rows.  Add --gather_top K (at most %d), run the samples one at a time, or drop --gather." % TOP_MAX_COHORT)


def gather_options(args, n_files: int = 1):
    """(coverages, min_hits) of a `yacht run --gather`, or None without the flag.  coverages: the --min_coverage_list values
    the ranking is made for, descending -- all of them, or the --gather_coverage ones.  ValueError when an option comes
    without --gather, names a coverage outside the list, asks for min_hits below 1, when --gather_top is refused (gather_top),
    or when there is more than one sample file and no --gather_top.  Host only: it runs before anything is written or any
    device work."""
    want = bool(getattr(args, "gather", False))
    covs = getattr(args, "gather_coverage", None)
    min_hits = getattr(args, "gather_min_hits", None)
    if not want:
        if covs is not None:
            raise ValueError(MSG_OPTION_WITHOUT_GATHER.format("--gather_coverage"))
        gather_top(args, n_files)
        return None
    if gather_top(args, n_files) is None and n_files > 1:
        raise ValueError(MSG_COHORT.format(n_files))
    min_hits = 1 if min_hits is None else int(min_hits)
    if min_hits < 1:
        raise ValueError(MSG_BAD_MIN_HITS.format(min_hits))
    listed = sorted(set(float(c) for c in args.min_coverage_list), reverse=True)
    if covs is None:
        return listed, min_hits
    covs = [float(c) for c in (covs if isinstance(covs, (list, tuple)) else [covs])]
    for c in covs:
        if c not in listed:
            raise ValueError(MSG_COVERAGE_NOT_LISTED.format(c, listed))
    return sorted(set(covs), reverse=True), min_hits


def gather_top(args, n_files: int = 1) -> Optional[int]:
    """K of `--gather_top K`: at most K organisms are ranked per sample and coverage (cap_rows of the ranking); None without
    the option.  ValueError when it comes without --gather, is below 1, or -- for a cohort -- above TOP_MAX_COHORT."""
    top = getattr(args, "gather_top", None)
    if top is None:
        return None
    if not bool(getattr(args, "gather", False)):
        raise ValueError(MSG_OPTION_WITHOUT_GATHER.format("--gather_top"))
    if int(top) < 1:
        raise ValueError(MSG_BAD_TOP.format(top))
    if n_files > 1 and int(top) > TOP_MAX_COHORT:
        raise ValueError(MSG_TOP_ABOVE_MAX.format(top, TOP_MAX_COHORT))
    return int(top)


def candidate_table(n_refs: int, call_set) -> np.ndarray:
    """The candidate table of RefDB.gather, uint8 [n_refs]: 1 at the manifest rows of one call set."""
    rows = np.asarray(call_set, dtype=np.int64)
    if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= int(n_refs)):
        raise ValueError(f"the call set names a row outside [0, {int(n_refs)})")
    table = np.zeros(int(n_refs), dtype=np.uint8)
    table[rows] = 1
    return table


def gather_call_sets(db, sample, abund, call_sets: Sequence, min_hits: int = 1, cap_rows: Optional[int] = None) -> List[np.ndarray]:
    """One RefDB.gather call per call set (arrays of manifest row indices): the rows of each, at most cap_rows (None: uncapped)."""
    return [db.gather(sample, candidate_table(db.n_refs, s), abund, min_hits=min_hits, cap_rows=cap_rows)[0] for s in call_sets]


def gather_frame(covs: Sequence[float], rows: Sequence, names, n_hashes: int, abund_total: int) -> pd.DataFrame:
    """One row per (coverage, rank), coverage descending, then rank (GATHER_COLUMNS).  covs[c] / rows[c]: the c-th coverage
    and RefDB.gather's rows for its call set, already in rank order; names: the manifest's organism names, indexed by a row's
    ref; n_hashes / abund_total: the size of the sample and the sum of its abundances (its size when the sketch has none).
    The fractions are over those two, 0 for an empty sample; mean_abund_unique = abund_sum_unique / num_unique."""
    names = np.asarray(names, dtype=object)
    n_hashes, abund_total = int(n_hashes), int(abund_total)
    out = []
    for cov, rws in zip(covs, rows):
        for rank, r in enumerate(rws):
            n_ov, n_un, w_un = int(r["n_overlap"]), int(r["n_unique"]), int(r["w_unique"])
            out.append((float(cov), rank, names[int(r["ref"])], n_ov, n_un,
                        n_ov / n_hashes if n_hashes else 0.0, n_un / n_hashes if n_hashes else 0.0,
                        w_un, w_un / n_un if n_un else 0.0, w_un / abund_total if abund_total else 0.0))
    out.sort(key=lambda t: (-t[0], t[1]))
    frame = pd.DataFrame(out, columns=GATHER_COLUMNS)
    return frame.astype({"rank": np.int64, "num_overlap": np.int64, "num_unique": np.int64}) if len(frame) else frame


def sample_frame(sample_sig, covs: Sequence[float], rows: Sequence, names) -> pd.DataFrame:
    """gather_frame for a sample's signature: the fractions are over its hashes and the sum of its abundances."""
    mh = sample_sig.minhash
    n_hashes = len(mh)
    abund_total = n_hashes if mh.abundances is None else int(np.asarray(mh.abundances, dtype=np.uint64).sum(dtype=np.uint64))
    return gather_frame(covs, rows, names, n_hashes, abund_total)


def write_frame(results_folder: str, frame: pd.DataFrame) -> None:
    frame.to_csv(os.path.join(results_folder, GATHER_NAME), sep="\t", index=False)


def write_profile(results_folder: str, sample_sig, covs: Sequence[float], rows: Sequence, names) -> pd.DataFrame:
    """results/gather_profile.tsv from the rows of every chosen coverage.  Returns the frame."""
    frame = sample_frame(sample_sig, covs, rows, names)
    write_frame(results_folder, frame)
    return frame


def cohort_frame(stems: Sequence[str], frames: Sequence[pd.DataFrame]) -> pd.DataFrame:
    """results/cohort_gather.tsv: the samples' gather_profile.tsv frames in long form, one after the other in the order
    given, behind a `sample` column.  No sample (or only empty frames): the columns alone."""
    parts = []
    for stem, frame in zip(stems, frames):
        if len(frame):
            part = frame.copy()
            part.insert(0, "sample", stem)
            parts.append(part)
    return pd.concat(parts, ignore_index=True) if parts else pd.DataFrame(columns=["sample"] + GATHER_COLUMNS)
