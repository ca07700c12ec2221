"""`yacht run` over a cohort: several samples against one trained database in one process.

The database is built once (hypothesis_recovery_src.get_reference_db).  Samples go to the device in blocks of up to
YH_BATCH_MAX_SAMPLES: one yh_run_batch_device per block, its compact rows (yh_run_batch_rows_pack/_unpack_device; the
dense rows when the row count exceeds the capacity) and the presence test of those rows on the device
(yh_presence_rows_device).  The acceptance threshold, confidence and alt. mutation rate depend on n alone: one yh_hyp_test
over n = 0..max reference size gives their table, gathered on the host by n_cov.  While block j is on the device the host
assembles block j - 1's tables (the single path's own helpers: coverage_frame, trim_results), host threads parse block
j + 1, and a pool of --num_threads processes writes the tables.

With --gather --gather_top K the block's ranking follows on the device (yh_explain_members_rows_device, then one
yh_gather_batch_device per gather coverage): results/<stem>/gather_profile.tsv and results/cohort_gather.tsv.

With --lineages --lineages_rank RANK the tree is built and set once, and per block one yh_lca_batch_device and one
yh_lca_rows_pack_device follow: results/<stem>/lca_summary.tsv and results/cohort_lca.tsv, cut at RANK (taxonomy.rank_rows).

With --matrix the block's rows some coverage calls present become cells that stay on the device (yh_matrix_cells_device), and
after the last block yh_matrix_prevalence_device and yh_matrix_fill_device make the organism x sample tables of
yacht_amd/matrix.py: results/cohort_prevalence.tsv and results/cohort_matrix_*.tsv.

Output: results/<stem>/ per sample with overlap (what a single-sample run of that file writes into results/),
results/cohort_samples.tsv and results/cohort_presence.tsv.  Every input is checked before any device work; the
per-sample intermediate files of the single path (multisearch CSV, list files) are not written.  Every sample is parsed
in that check (exactly one sketch of the database's k-mer size, its scale); only its size, mean abundance and scale are
kept, and the sketches are parsed again block by block, so host memory holds a few blocks of samples, not the cohort.
"""
from __future__ import annotations

import ctypes as C
import json
import multiprocessing
import os
import time
import zipfile
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
from pathlib import Path
from typing import Dict, List

import numpy as np
import pandas as pd

from . import _lib
from . import hypothesis_recovery_src as hr
from . import run_YACHT as ry
from . import utils
from .utils import logger

BLOCK = _lib.YH_BATCH_MAX_SAMPLES  # samples per yh_run_batch_device
MAX_COVS = _lib.YH_PRESENCE_MAX_COVS  # coverages per yh_presence_rows_device (more coverages take more launches)
MAX_SETS = 7  # call sets per explain pass: bits 0..6 of a member byte (residual.MAX_SETS)
# rows of a block's lineage counts the row buffer starts with at most (24 bytes each; a real-shape sample meets ~21 000 nodes);
# it grows after a block that exceeded it
LCA_ROWS_CAP = 1 << 23
SAMPLE_COLUMNS = ["stem", "path", "n_hashes", "mean_abundance", "n_overlapping", "status"]
PRESENCE_COLUMNS = ["sample", "min_coverage", "organism_name", "num_matches", "acceptance_threshold_with_coverage", "p_vals"]
PRESENCE_ABUNDANCE_COLUMNS = ["abund_median_exclusive", "relative_abundance"]  # behind them with --abundance


def sample_stem(path: str) -> str:
    """The sample's name as hypothesis_recovery derives it: the basename without .sig.zip."""
    return os.path.basename(path).replace(".sig.zip", "")


def _check_one(path: str, ksize: int):
    """(n_hashes, mean_abundance, scaled) of the sample's one sketch of this k-mer size, or the single path's error."""
    try:
        mh = utils.load_signature_with_ksize(path, ksize).minhash
    except ValueError:
        return None, ValueError(ry.MSG_NOT_ONE_SKETCH.format(path, ksize, len(path)))
    return (len(mh), mh.mean_abundance, mh.scaled), None


def _load_mins(path: str, ksize: int) -> np.ndarray:
    return np.ascontiguousarray(hr._sample_mins(utils.load_signature_with_ksize(path, ksize)), dtype=np.uint64)


def _load_mins_abund(path: str, ksize: int):
    """(hashes, their abundances as uint32) of a sample (--abundance)."""
    from . import abundance
    from .engine import check_abundances

    sig = utils.load_signature_with_ksize(path, ksize)
    return check_abundances(hr._sample_mins(sig), abundance.sample_abundances(sig, path))


def _load_for_residual(path: str, ksize: int, want_abundance: bool):
    """(hashes, their abundances as uint32 or None, the signature) of a sample (--residual): the abundances when the sketch
    tracks them, which --abundance insists on."""
    from . import abundance, residual
    from .engine import check_abundances

    sig = utils.load_signature_with_ksize(path, ksize)
    mins = np.ascontiguousarray(hr._sample_mins(sig), dtype=np.uint64)
    ab = abundance.sample_abundances(sig, path) if want_abundance else residual.sample_abundances_or_none(sig)
    return (mins, None, sig) if ab is None else (*check_abundances(mins, ab), sig)


def check_inputs(args, files: List[str]) -> dict:
    """Every check of the single path, for every file, before any device work and before anything is written: the
    config, the output location, the coverages, the manifest, distinct sample stems, and per file the archive's manifest,
    exactly one sketch of the database's k-mer size and its scale.  Returns what the run needs; of every sample only
    meta[i] = (n_hashes, mean_abundance, scaled)."""
    if getattr(args, "residual", False) or getattr(args, "residual_coverage", None) is not None:
        from . import residual

        residual.residual_coverage(args)
    if any(getattr(args, k, None) for k in ("gather", "gather_coverage", "gather_top")):
        from . import gather

        gather.gather_options(args, len(files))
    lineages = lineages_rank = None
    if getattr(args, "lineages", None) is not None or getattr(args, "lineages_rank", None) is not None:
        from . import taxonomy

        lineages = taxonomy.lineages_option(args, len(files))
        lineages_rank = taxonomy.lineages_rank(args)
    matrix_plan = None
    if getattr(args, "matrix", False) or any(getattr(args, k, None) is not None for k in ("matrix_coverage", "matrix_min_samples")):
        from . import matrix

        matrix_plan = matrix.matrix_options(args, len(files))
    json_file_path = str(Path(args.json).absolute())
    paths = [str(Path(f).absolute()) for f in files]
    outdir = str(Path(args.outdir).absolute())
    utils.check_file_existence(json_file_path, ry.MSG_NO_CONFIG.format(json_file_path))
    with open(json_file_path) as f:
        config = json.load(f)
    if not os.access(outdir, os.W_OK):
        raise PermissionError(f"Cannot write to the location: {outdir}.")
    for x in args.min_coverage_list:
        if not (0 <= x <= 1):
            raise ValueError(ry.MSG_BAD_COVERAGE.format(x))
    utils.check_file_existence(config["manifest_file_path"], ry.MSG_NO_MANIFEST.format(config["manifest_file_path"]))
    seen: Dict[str, str] = {}
    for p in paths:
        stem = sample_stem(p)
        if stem in seen:
            raise ValueError(f"Two sample files share the name {stem!r} (results/{stem}/): {seen[stem]} and {p}")
        seen[stem] = p
    for p in paths:
        with zipfile.ZipFile(p, "r") as z:
            if "SOURMASH-MANIFEST.csv" not in z.namelist():
                raise FileNotFoundError(ry.MSG_ZIP_WITHOUT_MANIFEST.format(p))
    ksize, scale = config["ksize"], config["scale"]
    with ThreadPoolExecutor(max(1, min(int(args.num_threads), len(paths)))) as ex:
        parsed = list(ex.map(lambda p: _check_one(p, ksize), paths))
    meta = []
    for p, (m, err) in zip(paths, parsed):
        if err is not None:
            raise err
        if m[2] != scale:
            raise ValueError(f"{ry.MSG_SCALE_MISMATCH} Sample: {p}")
        if getattr(args, "abundance", False) and m[1] is None:
            from . import abundance

            raise ValueError(abundance.MSG_NO_ABUNDANCE.format(p))
        meta.append(m)
    return dict(config=config, paths=paths, outdir=outdir, meta=meta, lineages=lineages, lineages_rank=lineages_rank, matrix=matrix_plan)


_LCA_TREE = None  # (parent, leaf, node_lineages) of --lineages in a process of the write pool: sent once, not with every sample


def _init_writer(tree) -> None:
    global _LCA_TREE
    _LCA_TREE = tree


def _write_one(folder: str, results, covs, has_raw: bool, keep_raw: bool, show_all: bool, profile: bool = False, explained=None,
               ranked=None, lineage=None):
    """One sample's files.  Returns its rows of cohort_lca.tsv (taxonomy.rank_rows) with --lineages, else None."""
    os.makedirs(folder, exist_ok=True)
    ry.write_sample_results(results, covs, has_raw, folder, keep_raw, show_all)
    if profile:
        from . import abundance

        abundance.write_profile(results if has_raw else results[1:], covs if has_raw else covs[1:], folder)
    if explained is not None:  # (sample signature, call sets, flags, totals, residual coverage) of --residual
        from . import residual

        sig, call_sets, flags, totals, cov = explained
        residual.write_outputs(folder, sig, covs if has_raw else covs[1:], call_sets, flags, totals, cov)
    if ranked is not None:  # the sample's gather_profile.tsv frame of --gather
        from . import gather

        gather.write_frame(folder, ranked)
    if lineage is not None:  # the sample's non-zero lineage counts (node, n_hashes, w_hashes), its size and abundance, call sets, rank
        from . import taxonomy

        nodes, n_h, w_h, n_hashes, abund_total, call_sets, rank = lineage
        parent, leaf, node_lineages = _LCA_TREE
        counts = np.zeros((len(parent), 2), dtype=np.uint64)
        counts[nodes, 0], counts[nodes, 1] = n_h, w_h
        taxonomy.write_summary(folder, taxonomy.summary_frame(parent, leaf, node_lineages, counts, n_hashes, abund_total,
                                                              covs if has_raw else covs[1:], call_sets))
        return taxonomy.rank_rows(parent, leaf, node_lineages, counts, rank, n_hashes, abund_total)
    return None


class _Device:
    """The device side of a cohort run: the block's buffers and the calls of one block."""

    def __init__(self, db, covs, ksize: int, ani_thresh: float, thr_table: np.ndarray, cap: int = 0, abund_samples: int = 0,
                 residual_sets: int = 0, gather_sets=(), gather_min_hits: int = 1, gather_top: int = 0, n_user: int = 0,
                 max_samples: int = BLOCK, lca_nodes: int = 0, lca_cap: int = 0, matrix_sets: int = 0):
        """cap: compact rows a block may have before it takes the dense rows (0: BLOCK * N, at most 2^20; grows after a
        block that exceeded it).  abund_samples (--abundance): samples of the largest block; 0 = no abundance pass.
        residual_sets (--residual): the number of user coverages, the LAST residual_sets entries of covs, whose call sets
        the block's explain passes answer, seven per pass; 0 = no explain pass.  gather_sets (--gather): which of the n_user
        user coverages (indices into them; they are the LAST n_user entries of covs) the block's ranking is made for, with
        gather_min_hits and at most gather_top rows per sample and coverage, for blocks of up to max_samples; empty = no
        ranking.  lca_nodes (--lineages): the nodes of the taxonomy set on db, for blocks of up to max_samples; 0 = no
        lineage pass.  lca_cap: rows of a block's lineage counts the row buffer starts with (0: LCA_ROWS_CAP, at most one
        per cell; it grows after a block that exceeded it).  matrix_sets (--matrix): the number of user coverages, the LAST
        matrix_sets entries of covs, whose present bytes become the masks of the block's cells (yh_matrix_cells_device); the
        cells of every collected block stay on the device in matrix_cells; 0 = no cells."""
        import torch

        self.torch = torch
        self.matrix_sets = int(matrix_sets)
        self.db = db
        self.dev = torch.device(f"cuda:{db.info()['device_id']}")
        self.covs = np.ascontiguousarray(covs, dtype=np.float64)
        self.ksize, self.ani = int(ksize), float(ani_thresh)
        self.thr = torch.from_numpy(np.ascontiguousarray(thr_table, dtype=np.float64)).to(self.dev)
        self.n_max = int(thr_table.size - 1)
        N = db.n_refs
        self.counts = torch.zeros((3, BLOCK, max(N, 1)), dtype=torch.int32, device=self.dev)
        self.n_rows = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.n_rows_host = torch.zeros(2, dtype=torch.int32).pin_memory()
        self._alloc(int(cap) if cap > 0 else min(BLOCK * max(N, 1), 1 << 20))
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        self.abund = None
        if abund_samples > 0:  # [samples][N] sums and medians of a block (yh_abund_batch_device, one call per block)
            # YACHT_COHORT_ABUND=loop: yh_abund_device once per sample, as before the batched pass (an A/B switch: same files)
            self.abund_loop = os.environ.get("YACHT_COHORT_ABUND") == "loop"
            shape = (int(abund_samples), max(N, 1))
            self.abund = (torch.zeros(shape, dtype=torch.int64, device=self.dev), torch.zeros(shape, dtype=torch.int64, device=self.dev),
                          torch.zeros(shape, dtype=torch.float64, device=self.dev))
            self.abund_rows = None
            self.ev_abund = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        self.residual_sets = int(residual_sets)
        self.gather_sets = [int(g) for g in gather_sets]
        self.d_x_abund = None
        if self.residual_sets > 0 or self.gather_sets:  # member rows [BLOCK][N] of up to seven call sets at a time
            self.members = torch.zeros((BLOCK, max(N, 1)), dtype=torch.uint8, device=self.dev)
        if self.gather_sets:  # per block and gather coverage: rows [samples][top], their counts and `more` bytes
            self.n_user = int(n_user)
            self.gather_min_hits, self.gather_top = int(gather_min_hits), int(gather_top)
            g, bmax = len(self.gather_sets), max(1, min(BLOCK, int(max_samples)))
            self.g_rows = torch.zeros((g, bmax, self.gather_top, 3), dtype=torch.int64, device=self.dev)
            self.g_n = torch.zeros((g, bmax), dtype=torch.int32, device=self.dev)
            self.g_more = torch.zeros((g, bmax), dtype=torch.uint8, device=self.dev)
            self.ev_gather = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        if self.residual_sets > 0:  # per block and pass of seven call sets: totals and flags
            if self.residual_sets > self.covs.size:
                raise ValueError(f"{self.residual_sets} call sets for {self.covs.size} coverages")
            self.x_passes = (self.residual_sets + MAX_SETS - 1) // MAX_SETS
            self.x_totals = torch.zeros((self.x_passes, BLOCK, 8, 2), dtype=torch.int64, device=self.dev)
            self.x_flags = None  # [passes][the block's hashes], made per block
            self.d_x_abund = None
            self.ev_explain = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        self.lca_nodes = int(lca_nodes)
        if self.lca_nodes > 0:  # per block: dense counts [samples][nodes][2] (16 bytes a cell), their non-zero cells as rows
            bmax = max(1, min(BLOCK, int(max_samples)))
            self.l_counts = torch.zeros((bmax, self.lca_nodes, 2), dtype=torch.int64, device=self.dev)
            self.l_n = torch.zeros(1, dtype=torch.int64, device=self.dev)
            self.l_n_host = torch.zeros(1, dtype=torch.int64).pin_memory()
            self._lca_alloc(int(lca_cap) if lca_cap > 0 else min(bmax * self.lca_nodes, LCA_ROWS_CAP))
            self.ev_lca = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        if self.matrix_sets > 0:  # per block: its cells (24 bytes each, at most one per compact row) and their count
            if self.matrix_sets > self.covs.size:
                raise ValueError(f"{self.matrix_sets} matrix coverages for {self.covs.size} coverages")
            self.m_n = torch.zeros(1, dtype=torch.int64, device=self.dev)
            self.m_n_host = torch.zeros(1, dtype=torch.int64).pin_memory()
            self.m_base = 0
            self.matrix_cells = []  # the collected blocks' cells, device-resident, in block order
            self.ev_matrix = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def matrix_pass(self, rows, d_n_rows: int, cap: int, out, med, cells) -> None:
        """The block's cells: one yh_matrix_cells_device over the rows, the user coverages' present bytes and (with
        --abundance) the medians gathered at the rows.  No host sync: the count stays on the device."""
        first = self.covs.size - self.matrix_sets  # (the forced 1.0 in front is no user coverage)
        self.db.matrix_cells_device(rows.data_ptr(), d_n_rows, cap, out[1][first].data_ptr(), self.matrix_sets,
                                    med.data_ptr() if med is not None else 0, self.m_base, cells.data_ptr(), self.m_n.data_ptr())

    def _lca_alloc(self, cap: int) -> None:
        self.l_cap = int(cap)
        self.l_rows = self.torch.zeros((self.l_cap, 3), dtype=self.torch.int64, device=self.dev)  # (engine.LCA_ROW_DTYPE: 24 bytes)

    def lca_pass(self, b: int, total: int) -> None:
        """The block's lineage counts: one yh_lca_batch_device over the uploaded block, then their non-zero cells as rows
        (yh_lca_rows_pack_device) and the row count on its way to the host.  No host sync."""
        d_abund = self.d_x_abund.data_ptr() if self.d_x_abund is not None else 0
        self.db.lca_batch_device(self.d_samples.data_ptr(), self.d_offs.data_ptr(), d_abund, b, total, 0, self.l_counts.data_ptr())
        self.db.lca_rows_pack_device(self.l_counts.data_ptr(), b, self.l_rows.data_ptr(), self.l_cap, self.l_n.data_ptr())

    def _alloc(self, cap: int) -> None:
        t = self.torch
        self.cap = int(cap)
        self.vals = t.zeros((self.cap, 3), dtype=t.int32, device=self.dev)
        self.rows = t.zeros((self.cap, 5), dtype=t.int32, device=self.dev)
        self.out = self._out(self.cap)
        if self.matrix_sets > 0:
            self.m_cells = t.zeros((self.cap, 3), dtype=t.int64, device=self.dev)  # (engine.MATRIX_CELL_DTYPE: 24 bytes)

    def _out(self, cap: int):
        t = self.torch
        nc = self.covs.size
        return (t.empty((nc, cap), dtype=t.float64, device=self.dev), t.empty((nc, cap), dtype=t.uint8, device=self.dev),
                t.empty((nc, cap), dtype=t.int32, device=self.dev))

    def presence(self, rows, d_n_rows: int, cap: int, out) -> None:
        """yh_presence_rows_device over the rows, MAX_COVS coverages per launch; out = (p_val, present, n_cov) [n_covs][cap]."""
        from . import _lib

        lib = _lib.load()
        for c0 in range(0, self.covs.size, MAX_COVS):
            cv = self.covs[c0:c0 + MAX_COVS]
            _lib.check(lib.yh_presence_rows_device(self.db._h, C.c_void_p(rows.data_ptr()), C.c_void_p(d_n_rows), cap, self.ksize,
                                                   self.ani, cv.ctypes.data_as(C.c_void_p), int(cv.size),
                                                   C.c_void_p(self.thr.data_ptr()), self.n_max,
                                                   C.c_void_p(out[0][c0].data_ptr()), C.c_void_p(out[1][c0].data_ptr()),
                                                   C.c_void_p(out[2][c0].data_ptr())))

    def abundance_pass(self, offs: np.ndarray, b: int) -> None:
        """The block's abundance pass: one yh_abund_batch_device over the uploaded block (YACHT_COHORT_ABUND=loop:
        yh_abund_device once per sample on its slice, as before the batched pass; the same values), then the three values
        of every compact row (sample, reference) gathered on the device."""
        w_ov, w_m, med = self.abund
        if self.abund_loop:
            for s in range(b):
                self.db.abundance_device(self.d_samples.data_ptr() + 8 * int(offs[s]), self.d_abund.data_ptr() + 4 * int(offs[s]),
                                         int(offs[s + 1] - offs[s]), w_ov[s].data_ptr(), w_m[s].data_ptr(), med[s].data_ptr())
        else:
            self.db.abundance_batch_device(self.d_samples.data_ptr(), self.d_offs.data_ptr(), self.d_abund.data_ptr(), b,
                                           int(offs[b]), w_ov.data_ptr(), w_m.data_ptr(), med.data_ptr())
        self.abund_rows = self.gather_abundance(self.rows, b)

    def gather_abundance(self, rows, b: int):
        """(w_overlap, w_match, med_match) at the rows' (sample, reference); rows behind the block's count are clamped
        into range and never read on the host."""
        w_ov, w_m, med = self.abund
        smp = rows[:, 0].long().clamp_(0, max(b - 1, 0))
        ref = rows[:, 1].long().clamp_(0, w_ov.shape[1] - 1)
        return w_ov[smp, ref], w_m[smp, ref], med[smp, ref]

    def explain_pass(self, rows, d_n_rows: int, cap: int, out, b: int, total: int) -> None:
        """The block's residual: per pass of up to seven user coverages, the samples' member rows from the rows' present
        bytes (yh_explain_members_rows_device) and one yh_explain_batch_device over the uploaded block."""
        first = self.covs.size - self.residual_sets  # (the forced 1.0 in front is no user coverage)
        d_abund = self.d_x_abund.data_ptr() if self.d_x_abund is not None else 0
        for p in range(self.x_passes):
            c0 = first + p * MAX_SETS
            self.db.explain_members_rows_device(rows.data_ptr(), d_n_rows, cap, out[1][c0].data_ptr(),
                                                min(MAX_SETS, self.covs.size - c0), b, self.members.data_ptr())
            self.db.explain_batch_device(self.d_samples.data_ptr(), self.d_offs.data_ptr(), d_abund, b, total,
                                         self.members.data_ptr(), self.x_flags[p].data_ptr(), self.x_totals[p].data_ptr())

    def gather_pass(self, rows, d_n_rows: int, cap: int, out, b: int, total: int) -> None:
        """The block's ranking: per pass of up to seven user coverages that holds a gather coverage, the samples' member rows
        from the rows' present bytes (yh_explain_members_rows_device), then one yh_gather_batch_device per gather coverage
        with that coverage's bit as cand_mask.  No host sync: the counts and `more` bytes stay on the device."""
        first = self.covs.size - self.n_user  # (the forced 1.0 in front is no user coverage)
        d_abund = self.d_x_abund.data_ptr() if self.d_x_abund is not None else 0
        for c0 in range(0, self.n_user, MAX_SETS):
            mine = [(g, u - c0) for g, u in enumerate(self.gather_sets) if c0 <= u < c0 + MAX_SETS]
            if not mine:
                continue
            self.db.explain_members_rows_device(rows.data_ptr(), d_n_rows, cap, out[1][first + c0].data_ptr(),
                                                min(MAX_SETS, self.n_user - c0), b, self.members.data_ptr())
            for g, bit in mine:
                self.db.gather_batch_device(self.d_samples.data_ptr(), self.d_offs.data_ptr(), d_abund, b, total, self.members.data_ptr(),
                                            1 << bit, self.gather_min_hits, self.g_rows[g].data_ptr(), self.gather_top, 0,
                                            self.g_n[g].data_ptr(), self.g_more[g].data_ptr())

    def _upload_sketch_abundances(self, mins, abunds, explain_abunds, total: int) -> None:
        """d_x_abund for the explain and gather passes: the block's abundances where the sketches track them (a sample
        without counts every hash once), None when no sample of the block does.  Once per block."""
        t = self.torch
        if self.d_x_abund is not None or self._x_abund_done:
            return
        self._x_abund_done = True
        if abunds is not None:
            self.d_x_abund = self.d_abund
        elif explain_abunds is not None and total and any(a is not None for a in explain_abunds):
            cat_ab = np.concatenate([np.ones(m.size, np.uint32) if a is None else np.ascontiguousarray(a, dtype=np.uint32)
                                     for m, a in zip(mins, explain_abunds)]).view(np.int32)
            self.d_x_abund = t.from_numpy(cat_ab).pin_memory().to(self.dev, non_blocking=True)

    def launch(self, mins: List[np.ndarray], abunds=None, explain_abunds=None, sample_base=None) -> int:
        """Queue one block: upload, batch counts, compact rows, presence test, row count to the host.  No host sync.
        abunds (--abundance): every sample's abundances.  explain_abunds (the explain pass without --abundance): per sample
        its abundances or None; a sample without counts every hash once.  sample_base (--matrix): the cohort index of the
        block's first sample (None: 0).
        Events on the caller's (legacy default) stream, which the handle's blocking stream orders against, split the
        block's device time into upload, counts + compact rows, and the presence kernel."""
        t = self.torch
        ev = self.ev
        ev[0].record()
        b = len(mins)
        offs = np.zeros(b + 1, dtype=np.int64)
        offs[1:] = np.cumsum([m.size for m in mins])
        cat = np.concatenate(mins).view(np.int64) if offs[-1] else np.zeros(1, np.int64)
        self.d_samples = t.from_numpy(cat).pin_memory().to(self.dev, non_blocking=True)
        self.d_offs = t.from_numpy(offs).pin_memory().to(self.dev, non_blocking=True)
        ev[1].record()
        c = self.counts
        self.db.run_batch_device(self.d_samples.data_ptr(), self.d_offs.data_ptr(), b, int(offs[-1]), c[0].data_ptr(),
                                 c[1].data_ptr(), c[2].data_ptr())
        self.db.run_batch_rows_pack_device(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), self.vals.data_ptr(), self.cap,
                                           self.n_rows[0].data_ptr())
        self.db.run_batch_rows_unpack_device(self.vals.data_ptr(), self.cap, self.rows.data_ptr(), self.n_rows[1].data_ptr())
        ev[2].record()
        self.presence(self.rows, self.n_rows[1].data_ptr(), self.cap, self.out)
        ev[3].record()
        if abunds is not None:
            cat_ab = np.concatenate(abunds).view(np.int32) if offs[-1] else np.zeros(1, np.int32)
            self.d_abund = t.from_numpy(cat_ab).pin_memory().to(self.dev, non_blocking=True)
            self.ev_abund[0].record()
            self.abundance_pass(offs, b)
            self.ev_abund[1].record()
        if self.matrix_sets > 0:  # (behind the presence test and the abundance pass: their outputs are its inputs)
            self.m_base = int(sample_base or 0)
            self.ev_matrix[0].record()
            self.matrix_pass(self.rows, self.n_rows[1].data_ptr(), self.cap, self.out,
                             self.abund_rows[2] if self.abund is not None else None, self.m_cells)
            self.ev_matrix[1].record()
            self.m_n_host.copy_(self.m_n, non_blocking=True)
        total = int(offs[-1])
        self.x_block = (b, total)
        self.d_x_abund, self._x_abund_done = None, False
        if self.residual_sets > 0:
            self.x_flags = t.empty((self.x_passes, max(total, 1)), dtype=t.uint8, device=self.dev)
            self.ev_explain[0].record()  # (the upload of a mixed cohort's abundances below belongs to the pass)
            self._upload_sketch_abundances(mins, abunds, explain_abunds, total)
            self.explain_pass(self.rows, self.n_rows[1].data_ptr(), self.cap, self.out, b, total)
            self.ev_explain[1].record()
        if self.gather_sets:
            self.ev_gather[0].record()  # (likewise, when no explain pass uploaded them)
            self._upload_sketch_abundances(mins, abunds, explain_abunds, total)
            self.gather_pass(self.rows, self.n_rows[1].data_ptr(), self.cap, self.out, b, total)
            self.ev_gather[1].record()
        if self.lca_nodes > 0:
            self.ev_lca[0].record()  # (likewise)
            self._upload_sketch_abundances(mins, abunds, explain_abunds, total)
            self.lca_pass(b, total)
            self.ev_lca[1].record()
            self.l_n_host.copy_(self.l_n, non_blocking=True)
        self.n_rows_host.copy_(self.n_rows, non_blocking=True)
        return b

    def collect(self, b: int, timer: Dict[str, float]):
        """Wait for the block; its rows and the presence results on the host (dense rows when the capacity was short)."""
        t = self.torch
        t0 = time.perf_counter()
        self.db.synchronize()
        t.cuda.synchronize(self.dev)
        timer["device_wait"] += time.perf_counter() - t0
        ev = self.ev
        timer["gpu_h2d"] += ev[0].elapsed_time(ev[1]) / 1e3
        timer["gpu_counts"] += ev[1].elapsed_time(ev[2]) / 1e3
        timer["gpu_presence"] += ev[2].elapsed_time(ev[3]) / 1e3
        if self.abund is not None:
            timer["gpu_abund"] += self.ev_abund[0].elapsed_time(self.ev_abund[1]) / 1e3
        if self.residual_sets > 0:
            timer["gpu_explain"] += self.ev_explain[0].elapsed_time(self.ev_explain[1]) / 1e3
        if self.gather_sets:
            timer["gpu_gather"] += self.ev_gather[0].elapsed_time(self.ev_gather[1]) / 1e3
        k = int(self.n_rows_host[0])
        rows, out = self.rows, self.out
        abund_rows = self.abund_rows if self.abund is not None else None
        if self.matrix_sets > 0:
            timer["gpu_matrix"] += self.ev_matrix[0].elapsed_time(self.ev_matrix[1]) / 1e3
            m_cells, m_n = self.m_cells, int(self.m_n_host[0])
        if k > self.cap:  # more entries than the compact buffers hold: the block's rows from its dense counts
            ev[0].record()
            ov = self.counts[0, :b]
            idx = t.nonzero(ov.t() > 0)  # (reference, sample) order, as the compact rows
            ref, smp = idx[:, 0], idx[:, 1]
            rows = t.stack([smp, ref, ov[smp, ref], self.counts[1, smp, ref], self.counts[2, smp, ref]], dim=1).to(t.int32).contiguous()
            k = int(rows.shape[0])
            d_k = t.tensor([k], dtype=t.int32, device=self.dev)
            out = self._out(k)
            ev[1].record()
            self.presence(rows, d_k.data_ptr(), k, out)
            ev[2].record()
            if self.abund is not None:
                abund_rows = self.gather_abundance(rows, b)
            if self.residual_sets > 0:  # (the member rows came from the truncated rows: again from these)
                self.ev_explain[0].record()
                self.explain_pass(rows, d_k.data_ptr(), k, out, b, self.x_block[1])
                self.ev_explain[1].record()
            if self.gather_sets:  # (and the ranking's candidates)
                self.ev_gather[0].record()
                self.gather_pass(rows, d_k.data_ptr(), k, out, b, self.x_block[1])
                self.ev_gather[1].record()
            if self.matrix_sets > 0:  # (and the cells)
                m_cells = t.zeros((max(k, 1), 3), dtype=t.int64, device=self.dev)
                self.ev_matrix[0].record()
                self.matrix_pass(rows, d_k.data_ptr(), k, out, abund_rows[2] if abund_rows is not None else None, m_cells)
                self.ev_matrix[1].record()
            t0 = time.perf_counter()
            t.cuda.synchronize(self.dev)
            timer["device_wait"] += time.perf_counter() - t0
            if self.matrix_sets > 0:
                timer["gpu_matrix"] += self.ev_matrix[0].elapsed_time(self.ev_matrix[1]) / 1e3
                m_n = int(self.m_n.item())
            timer["gpu_counts"] += ev[0].elapsed_time(ev[1]) / 1e3
            timer["gpu_presence"] += ev[1].elapsed_time(ev[2]) / 1e3
            if self.residual_sets > 0:
                timer["gpu_explain"] += self.ev_explain[0].elapsed_time(self.ev_explain[1]) / 1e3
            if self.gather_sets:
                timer["gpu_gather"] += self.ev_gather[0].elapsed_time(self.ev_gather[1]) / 1e3
            timer["dense_fallback_blocks"] += 1
            self._alloc(int(k * 1.25) + 1)  # (the next blocks: compact rows again)
        if self.matrix_sets > 0:  # the block's cells stay on the device: one device-to-device copy behind the earlier blocks'
            self.matrix_cells.append(m_cells[:m_n].clone())
        t0 = time.perf_counter()
        got = (rows[:k].cpu().numpy().view(np.uint32), out[0][:, :k].cpu().numpy(), out[1][:, :k].cpu().numpy(),
               out[2][:, :k].cpu().numpy().view(np.uint32))
        if abund_rows is not None:
            got += ((abund_rows[0][:k].cpu().numpy().view(np.uint64), abund_rows[1][:k].cpu().numpy().view(np.uint64),
                     abund_rows[2][:k].cpu().numpy()),)
        if self.residual_sets > 0:  # flags [passes][the block's hashes], totals [passes][b][8][2]
            got += ((self.x_flags[:, :self.x_block[1]].cpu().numpy(), self.x_totals[:, :b].cpu().numpy().view(np.uint64)),)
        if self.gather_sets:  # counts [gather coverages][b] and rows [gather coverages][b][the longest ranking]
            from .engine import GATHER_ROW_DTYPE

            g_n = self.g_n[:, :b].cpu().numpy().view(np.uint32)
            longest = int(g_n.max()) if g_n.size else 0
            g_rows = self.g_rows[:, :b, :longest].contiguous().cpu().numpy().reshape(len(self.gather_sets), b, longest * 3)
            got += ((g_rows.view(GATHER_ROW_DTYPE), g_n),)
        timer["d2h"] += time.perf_counter() - t0
        if self.lca_nodes > 0:  # the block's lineage rows in (sample, node) order: always the LAST entry
            from .engine import LCA_ROW_DTYPE

            timer["gpu_lca"] += self.ev_lca[0].elapsed_time(self.ev_lca[1]) / 1e3
            k = int(self.l_n_host[0])
            if k > self.l_cap:  # more non-zero cells than the row buffer holds: the dense counts are still resident, pack them again
                self._lca_alloc(int(k * 1.25) + 1)  # (the next blocks start with this capacity)
                self.ev_lca[0].record()
                self.db.lca_rows_pack_device(self.l_counts.data_ptr(), b, self.l_rows.data_ptr(), self.l_cap, self.l_n.data_ptr())
                self.ev_lca[1].record()
                t0 = time.perf_counter()
                self.db.synchronize()
                t.cuda.synchronize(self.dev)
                timer["device_wait"] += time.perf_counter() - t0
                timer["gpu_lca"] += self.ev_lca[0].elapsed_time(self.ev_lca[1]) / 1e3
                timer["lca_repacked_blocks"] += 1
            t0 = time.perf_counter()
            got += (self.l_rows[:k].cpu().numpy().reshape(-1).view(LCA_ROW_DTYPE),)
            timer["d2h"] += time.perf_counter() - t0
        return got


def main(args, files: List[str]) -> dict:
    """The cohort form of `yacht run` (run_YACHT.main with two or more --sample_file).  Returns seconds per phase:
    check (every input, samples parsed once), db (database build), table (the per-n threshold table), device_setup (torch
    and the device buffers), parse_wait (the loop waiting for a block's sketches), device_wait (the loop waiting for a
    block's device work), gpu_h2d / gpu_counts / gpu_presence (device time of the uploads, the batch counts + compact rows,
    the presence kernel), gpu_abund (with --abundance: the block's yh_abund_batch_device call -- its yh_abund_device calls under
    YACHT_COHORT_ABUND=loop -- and the gather of their values at the compact rows), gpu_explain (with --residual: device time of the block's member-row and batched explain passes, plus
    the wall time of the host-form yh_explain calls of samples whose tables the host recomputed, or of every sample under
    YACHT_COHORT_EXPLAIN=host), gpu_gather (with --gather: device time of the block's member-row passes and batched rankings, plus
    the wall time of the host-form yh_gather calls of samples whose tables the host recomputed, or of every sample under
    YACHT_COHORT_GATHER=loop), gpu_lca and lca_repacked_blocks (only with --lineages: device time of the block's
    yh_lca_batch_device and rows pack -- under YACHT_COHORT_LCA=loop the HOST WALL time of every sample's host-form yh_lca call,
    not device time -- and the blocks whose rows were packed a second time into a larger buffer), gpu_compare (only with
    --compare: the HOST WALL time of the host-form yh_compare calls after the blocks, uploads and downloads included), gpu_matrix and matrix_files (only with --matrix: device time of the blocks' cell passes and of
    the prevalence and fill passes after the last block -- 0 under YACHT_COHORT_MATRIX=host -- and the host time of writing the
    tables), d2h, assemble, writes (what the write pool had left after the last block), cohort_files (the two
    cohort tables), total."""
    timer = {k: 0.0 for k in ("check", "db", "table", "device_setup", "parse_wait", "device_wait", "gpu_h2d", "gpu_counts",
                              "gpu_presence", "gpu_abund", "gpu_explain", "gpu_gather", "d2h", "assemble", "writes", "cohort_files", "dense_fallback_blocks", "total")}
    t_all = time.perf_counter()
    t0 = time.perf_counter()
    plan = check_inputs(args, files)
    timer["check"] = time.perf_counter() - t0
    config, paths, meta = plan["config"], plan["paths"], plan["meta"]
    genome_dir, ksize, ani_thresh = config["intermediate_files_dir"], config["ksize"], config["ani_thresh"]
    significance = args.significance
    covs, has_raw = ry.coverage_plan(args.min_coverage_list)
    user_covs = covs if has_raw else covs[1:]
    results_folder = os.path.join(plan["outdir"], "results")
    os.makedirs(results_folder, exist_ok=True)
    manifest = pd.read_csv(config["manifest_file_path"], sep="\t", header=0)
    names = manifest["organism_name"].to_numpy()
    dup_names = bool(manifest["organism_name"].duplicated().any())
    ry.decompress_legacy_db(genome_dir, args.num_threads)

    t0 = time.perf_counter()
    db = hr.get_reference_db(manifest, genome_dir, ksize, args.num_threads)
    timer["db"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    n_max = int(np.max(db.sizes)) if db.n_refs else 0
    tab = hr.hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, dtype=np.int64), ksize, significance, ani_thresh, 1.0)
    t_thr, t_conf, t_alt = tab[5], tab[6], tab[7]
    timer["table"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_abundance = bool(getattr(args, "abundance", False))
    if want_abundance:
        from . import abundance
    want_residual = bool(getattr(args, "residual", False))
    if want_residual:
        from . import residual

        residual_cov = residual.residual_coverage(args)
    # YACHT_COHORT_EXPLAIN=host: every sample's residual by its own host-form yh_explain call, as before the batched pass
    # (A/B checks); otherwise only the samples whose tables the host recomputed below take it
    device_explain = want_residual and os.environ.get("YACHT_COHORT_EXPLAIN") != "host"
    want_compare = bool(getattr(args, "compare", False))
    if want_compare:  # after the blocks: the samples against one another (compare.run_files)
        from . import compare

        timer["gpu_compare"] = 0.0
        # with --residual: per sample, 1 where the call set of --residual_coverage explains the hash (None: no overlap, nothing explained)
        compare_keeps = [None] * len(paths) if want_residual else None
    gather_plan = None
    if getattr(args, "gather", False):
        from . import gather

        gather_plan = gather.gather_options(args, len(paths))  # (coverages, min_hits)
        gather_top = gather.gather_top(args, len(paths))
        gather_idx = [[float(c) for c in user_covs].index(c) for c in gather_plan[0]]  # which user coverages are ranked
        gather_frames = []  # (stem, the sample's gather_profile.tsv frame), in cohort order
    # YACHT_COHORT_GATHER=loop: every sample's ranking by its own host-form yh_gather calls (A/B checks); otherwise only
    # the samples whose tables the host recomputed below take them
    device_gather = gather_plan is not None and os.environ.get("YACHT_COHORT_GATHER") != "loop"
    lineages, lca_rank = plan["lineages"], plan["lineages_rank"]
    tree = None
    if lineages is not None:  # the tree once from the manifest, set once on the resident database (references in manifest order)
        from . import taxonomy

        tree = taxonomy.build_tree(manifest["organism_name"], lineages)
        db.set_taxonomy(*tree[:3])
        lca_parts = []  # (stem, the sample's rows of cohort_lca.tsv or the future that returns them), in cohort order
        timer["gpu_lca"] = timer["lca_repacked_blocks"] = 0.0
    # YACHT_COHORT_LCA=loop: every sample's lineage counts by its own host-form yh_lca call (A/B checks; the same files)
    device_lca = tree is not None and os.environ.get("YACHT_COHORT_LCA") != "loop"
    matrix_plan = plan["matrix"]  # (--matrix_coverage, --matrix_min_samples, YACHT_COHORT_MATRIX=host) or None
    mcol = None
    if matrix_plan is not None:  # the organism x sample tables: the blocks' cells stay on the device (matrix.Collector)
        from . import matrix

        timer["gpu_matrix"] = timer["matrix_files"] = 0.0
        mcol = matrix.Collector(db.n_refs, len(paths), len(user_covs), want_abundance, matrix_plan[2])
    device_matrix = mcol is not None and not matrix_plan[2]
    dev = _Device(db, covs, ksize, ani_thresh, t_thr, abund_samples=min(BLOCK, len(paths)) if want_abundance else 0,
                  residual_sets=len(user_covs) if device_explain else 0,
                  **{**(dict(gather_sets=gather_idx, gather_min_hits=gather_plan[1], gather_top=gather_top, n_user=len(user_covs),
                             max_samples=len(paths)) if device_gather else {}),
                     **(dict(lca_nodes=len(tree[0]), max_samples=len(paths)) if device_lca else {}),
                     **(dict(matrix_sets=len(user_covs)) if device_matrix else {})})
    timer["device_setup"] = time.perf_counter() - t0

    blocks = [list(range(i, min(i + BLOCK, len(paths)))) for i in range(0, len(paths), BLOCK)]
    summary, presence = [], []
    presence_columns = PRESENCE_COLUMNS + (PRESENCE_ABUNDANCE_COLUMNS if want_abundance else [])
    ctx = multiprocessing.get_context("spawn")  # (the parent holds the GPU: no fork)
    pool = ProcessPoolExecutor(max_workers=max(1, int(args.num_threads)), mp_context=ctx,
                               **(dict(initializer=_init_writer, initargs=((tree[0], tree[2], tree[3]),)) if tree is not None else {}))
    futures = []
    parse_pool = ThreadPoolExecutor(max(1, int(args.num_threads)))
    want_sigs = want_residual or gather_plan is not None or tree is not None  # (the passes that take a sketch's own abundances)

    def parse(block):
        if want_sigs:
            return [parse_pool.submit(_load_for_residual, paths[i], ksize, want_abundance) for i in block]
        return [parse_pool.submit(_load_mins_abund if want_abundance else _load_mins, paths[i], ksize) for i in block]

    def assemble(block, mins, got, abunds=None, sigs=None):
        rows, pv, pres, ncov = got[:4]
        t0 = time.perf_counter()
        if device_lca:  # the block's lineage rows, ascending (sample, node): the last entry, taken off before the others are read
            l_rows, got = got[-1], got[:-1]
            l_bounds = np.searchsorted(l_rows["sample"], np.arange(len(block) + 1))
        if device_gather:  # the block's rows [gather coverages][samples][longest ranking] and their counts
            g_rows, g_n = got[-1]
        if device_explain:  # the block's flags [passes][hashes] and totals [passes][samples][8][2]
            x_flags, x_totals = got[-2 if device_gather else -1]
            x_offs = np.zeros(len(block) + 1, dtype=np.int64)
            x_offs[1:] = np.cumsum([m.size for m in mins])
        smp = rows[:, 0]
        order = np.argsort(smp, kind="stable")  # per sample, references ascending (the rows are in (reference, sample) order)
        bounds = np.searchsorted(smp[order], np.arange(len(block) + 1))
        for s, i in enumerate(block):
            sel = order[bounds[s]:bounds[s + 1]]
            n_hashes, mean_abundance, scaled = meta[i]
            stem = sample_stem(paths[i])
            summary.append([stem, paths[i], n_hashes, mean_abundance, int(sel.size), "ok" if sel.size else "no_overlap"]
                           + ([0.0, 0.0] if want_residual else []))  # (no overlap: nothing explained, and no device call)
            if tree is not None:  # the sum of the sketch's own abundances, its size when it tracks none
                lca_total = n_hashes if abunds[s] is None else int(np.asarray(abunds[s], dtype=np.uint64).sum(dtype=np.uint64))
            if not sel.size:
                if tree is not None:  # (no reference holds a hash of it: its not_in_database row alone)
                    lca_parts.append((stem, taxonomy.no_overlap_rows(n_hashes, lca_total)))
                continue
            refs = rows[sel, 1].astype(np.int64)
            e = rows[sel, 3].astype(np.int64)
            m = rows[sel, 4].astype(np.int64)
            cols = None
            recomputed = False  # the dup_names branch below made this sample's tables on the host
            if want_abundance:  # the device's three values and the overlap count of the sample's rows
                depth = [got[4][0][sel], got[4][1][sel], got[4][2][sel], rows[sel, 2]]
            if dup_names:  # get_exclusive_hashes selects by NAME: a reference without overlap may share a name with one that has it
                selected = np.isin(names, names[refs])
                if int(selected.sum()) != refs.size:
                    ex_e, ex_m = db.exclusive(selected, mins[s])
                    if want_abundance:  # references pulled in by name have no overlap: sums 0, means and median NaN
                        at = np.searchsorted(np.flatnonzero(selected), refs)
                        wide = [np.zeros(int(selected.sum()), dtype=a.dtype) for a in depth]
                        for w, a in zip(wide, depth):
                            w[at] = a
                        depth = wide
                    refs = np.flatnonzero(selected)
                    e, m = ex_e[refs].astype(np.int64), ex_m[refs].astype(np.int64)
                    test = hr.hyp_test_native if os.environ.get("YACHT_HYP_NATIVE") == "1" else hr.hyp_test_batch
                    cols = [test(e, m, ksize, significance, ani_thresh, cov) for cov in covs]
                    recomputed = True
            if cols is None:
                cols = []
                for c in range(len(covs)):
                    nc = ncov[c, sel].astype(np.int64)
                    cols.append((pres[c, sel].astype(bool), pv[c, sel], e, nc, m, t_thr[nc], t_conf[nc], t_alt[nc]))
            sub = manifest.iloc[refs].reset_index(drop=True)
            ry.add_sample_columns(sub, mean_abundance, n_hashes, scaled)
            frames = [hr.coverage_frame(sub, col, cov) for col, cov in zip(cols, covs)]
            if want_abundance:
                total = int(abunds[s].sum(dtype=np.uint64))
                frames = [abundance.append_columns(f, *depth, total) for f in frames]
            frames = ry.trim_results(frames)
            if mcol is not None and (recomputed or not device_matrix):  # (the device's cells of a recomputed sample are skipped)
                mcol.add_host(i, refs, frames if has_raw else frames[1:])
            explained = ranked = lineage = None
            if want_sigs:
                call_sets = [refs[df["in_sample_est"].to_numpy().astype(bool)] for df in (frames if has_raw else frames[1:])]
            if gather_plan is not None:
                if device_gather and not recomputed:  # the device's present bytes ARE these call sets: the block's ranking
                    ranks = [g_rows[g, s, :int(g_n[g, s])] for g in range(len(gather_idx))]
                else:  # the host's own tables: one host-form call per gather coverage
                    t1 = time.perf_counter()
                    ranks = gather.gather_call_sets(db, mins[s], abunds[s] if abunds is not None else None,
                                                    [call_sets[u] for u in gather_idx], gather_plan[1], gather_top)
                    timer["gpu_gather"] += time.perf_counter() - t1
                ranked = gather.sample_frame(sigs[s], gather_plan[0], ranks, names)
                gather_frames.append((stem, ranked))
            if want_residual:
                if device_explain and not recomputed:  # the device's present bytes ARE these call sets: the block's pass answered them
                    flags = [x_flags[c // MAX_SETS, x_offs[s]:x_offs[s + 1]] for c in range(len(call_sets))]
                    totals = [x_totals[c // MAX_SETS, s] for c in range(len(call_sets))]
                else:  # the host's own tables: one host-form call per seven coverages
                    t1 = time.perf_counter()
                    flags, totals = residual.explain_call_sets(db, mins[s], abunds[s] if abunds is not None else None, call_sets)
                    timer["gpu_explain"] += time.perf_counter() - t1
                mh = sigs[s].minhash
                total = n_hashes if mh.abundances is None else int(np.asarray(mh.abundances, dtype=np.uint64).sum(dtype=np.uint64))
                row = residual.explained_frame(user_covs, [len(c) for c in call_sets], totals, n_hashes, total)
                row = row[row["min_coverage"] == residual_cov].iloc[0]
                summary[-1][-2:] = [float(row["f_hashes_explained"]), float(row["f_abund_explained"])]
                explained = (sigs[s], call_sets, flags, totals, residual_cov)
                if want_compare:  # the bit residual.write_outputs cuts residual.sig.zip by
                    c = [float(x) for x in user_covs].index(float(residual_cov))
                    compare_keeps[i] = ((np.asarray(flags[c], dtype=np.uint8) >> np.uint8(c % MAX_SETS)) & np.uint8(1)).astype(np.uint8)
            if tree is not None:  # the sample's non-zero lineage counts; the write pool makes its table and its rows of the cohort's
                if device_lca:
                    mine = l_rows[l_bounds[s]:l_bounds[s + 1]]
                    at, n_h, w_h = mine["node"].astype(np.int64), mine["n_hashes"].copy(), mine["w_hashes"].copy()
                else:
                    t1 = time.perf_counter()
                    dense = db.lca(mins[s], abunds[s], want_nodes=False)[1]
                    timer["gpu_lca"] += time.perf_counter() - t1  # (host wall time of the call, not device time)
                    at = np.flatnonzero(dense[:, 0])
                    n_h, w_h = dense[at, 0], dense[at, 1]
                lineage = (at, n_h, w_h, n_hashes, lca_total, call_sets, lca_rank)
            for cov, df in zip(user_covs, frames if has_raw else frames[1:]):
                hit = df[df["in_sample_est"] == True]  # noqa: E712
                if len(hit):
                    part = {"sample": stem, "min_coverage": cov, "organism_name": hit["organism_name"].to_numpy(),
                            "num_matches": hit["num_matches"].to_numpy(),
                            "acceptance_threshold_with_coverage": hit["acceptance_threshold_with_coverage"].to_numpy(),
                            "p_vals": hit["p_vals"].to_numpy()}
                    for c in PRESENCE_ABUNDANCE_COLUMNS if want_abundance else ():
                        part[c] = hit[c].to_numpy()
                    presence.append(pd.DataFrame(part, columns=presence_columns))
            futures.append(pool.submit(_write_one, os.path.join(results_folder, stem), frames, covs, has_raw, args.keep_raw,
                                       args.show_all, want_abundance, explained, ranked, lineage))
            if tree is not None:
                lca_parts.append((stem, futures[-1]))
        timer["assemble"] += time.perf_counter() - t0

    try:
        logger.info(f"Running {len(paths)} samples in {len(blocks)} block(s) of up to {BLOCK}.")
        pending = None
        parsing = parse(blocks[0]) if blocks else []
        for j, block in enumerate(blocks):
            t0 = time.perf_counter()
            mins = [f.result() for f in parsing]
            abunds = sigs = None
            if want_sigs:  # (abundances where the sketch tracks them; --abundance has checked that every one does)
                mins, abunds, sigs = [x[0] for x in mins], [x[1] for x in mins], [x[2] for x in mins]
            elif want_abundance:
                mins, abunds = [x[0] for x in mins], [x[1] for x in mins]
            timer["parse_wait"] += time.perf_counter() - t0
            parsing = parse(blocks[j + 1]) if j + 1 < len(blocks) else []
            b = dev.launch(mins, abunds if want_abundance else None, abunds if (device_explain or device_gather or device_lca) and not want_abundance else None,
                           **(dict(sample_base=block[0]) if device_matrix else {}))
            if pending is not None:
                assemble(*pending)  # (block j - 1 on the host while block j is on the device and block j + 1 is parsed)
            pending = (block, mins, dev.collect(b, timer), abunds, sigs)
        if pending is not None:
            assemble(*pending)
        t0 = time.perf_counter()
        for f in futures:
            f.result()
        timer["writes"] = time.perf_counter() - t0  # (the part of the writes not hidden behind the device and the assembly)
        if mcol is not None:  # (while the database is resident: the passes are enqueued on its handle)
            for cells in dev.matrix_cells if device_matrix else ():
                mcol.add_device(cells)
            mcol.finish(results_folder, names, [sample_stem(p) for p in paths], user_covs, matrix_plan[0], matrix_plan[1],
                        db, dev.torch, dev.dev, timer)
    finally:
        parse_pool.shutdown(wait=True)
        pool.shutdown(wait=True)
        hr.release_reference_dbs()
    t0 = time.perf_counter()
    pd.DataFrame(summary, columns=SAMPLE_COLUMNS + (residual.COHORT_COLUMNS if want_residual else [])).to_csv(os.path.join(results_folder, "cohort_samples.tsv"), sep="\t", index=False)
    (pd.concat(presence, ignore_index=True) if presence else pd.DataFrame(columns=presence_columns)).to_csv(
        os.path.join(results_folder, "cohort_presence.tsv"), sep="\t", index=False)
    if gather_plan is not None:
        gather.cohort_frame([g[0] for g in gather_frames], [g[1] for g in gather_frames]).to_csv(
            os.path.join(results_folder, gather.COHORT_GATHER_NAME), sep="\t", index=False)
    if tree is not None:
        taxonomy.cohort_frame([p[0] for p in lca_parts], [p[1] if isinstance(p[1], list) else p[1].result() for p in lca_parts]).to_csv(
            os.path.join(results_folder, taxonomy.COHORT_NAME), sep="\t", index=False)
    timer["cohort_files"] = time.perf_counter() - t0
    if want_compare:  # (the database is released: the samples, parsed again panel by panel, have the device to themselves)
        timer["gpu_compare"] = compare.run_files(paths, [sample_stem(p) for p in paths], meta, ksize, results_folder, args.num_threads,
                                                 compare_keeps)
    timer["total"] = time.perf_counter() - t_all
    logger.info(f"Saved results of {len(paths)} samples to {results_folder}.")
    return timer
