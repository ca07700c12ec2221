#!/usr/bin/env python3
"""Device time of the organism x sample passes (yh_matrix_cells_device, yh_matrix_prevalence_device, yh_matrix_fill_device)
next to the numpy route over the same cells (yacht_amd/matrix.py: what YACHT_COHORT_MATRIX=host builds the tables with).

    python scripts/bench_matrix.py [--n-refs 85205] [--samples 1024] [--rounds 3] [--out FILE]

On the synthetic database at GTDB rs214 scale (synth.config3_device), --samples real-shape 83 k-hash samples with abundances
(synth.sample_device) go through cohort._Device in blocks of 256 with five coverages, as `yacht run --abundance --matrix` sends
them; every block's rows, present bytes and medians are kept on the device.  Before anything is timed the device's cells of
every block must equal matrix.cells_from_rows of the same block, and its prevalence counts, depth sums and the three wide
matrices of the smallest coverage (every organism present in a sample kept) must equal matrix.prevalence_numpy and
matrix.fill_numpy on those cells.  Timed, alternating inside each of --rounds rounds: (a) HIP events on the caller's stream around
the blocks' cell passes, the prevalence pass and the fill, their buffers allocated beforehand; (b) the host wall time of
prevalence_numpy + fill_numpy on the cells.  The per-coverage abundance statistics of cohort_prevalence.tsv are further fill
passes and numpy reductions that both routes share; they are in neither figure.  The median round is reported with the
spread, and the expectation -- the device no slower than numpy -- is judged at the larger of 10 % and the rounds' spread.
Prints one JSON line and writes it to --out (default profiles/matrix/bench_matrix.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yacht_amd import _lib, cohort, matrix, synth  # noqa: E402
from yacht_amd.engine import MATRIX_CELL_DTYPE, RefDB  # noqa: E402
from yacht_amd.hypothesis_recovery_src import hyp_test_native  # noqa: E402

COVS = [1.0, 0.5, 0.1, 0.05, 0.01]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--sample-hashes", type=int, default=83_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cap-rows", type=int, default=1 << 23)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "matrix",
                                                  "bench_matrix.json"))
    a = ap.parse_args()
    import torch

    assert _lib.device_count() >= 1, "bench_matrix.py needs an MI355X"
    t = torch
    N, S, n_sets, bit = a.n_refs, a.samples, len(COVS), len(COVS) - 1
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    sizes = np.diff(offsets.cpu().numpy()).astype(np.uint32)
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N, sizes=sizes)
    n_max = int(sizes.max())
    tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
    # (a block of 256 real-shape samples has ~7 x 10^6 rows: room for them, so that no block takes the dense fallback)
    dev = cohort._Device(db, COVS, 31, 0.95, tab[5], cap=a.cap_rows, abund_samples=min(cohort.BLOCK, S), matrix_sets=n_sets)
    rng = np.random.default_rng(7)
    t_setup = time.perf_counter()
    blocks = []  # per block: (first sample, rows, their count, present bytes, medians, capacity), clones on the device
    timer = defaultdict(float)
    for lo in range(0, S, cohort.BLOCK):
        mins = [synth.sample_device(values, offsets, seed=4000 + i, n_sample=a.sample_hashes, shape="real").cpu().numpy().view(np.uint64)
                for i in range(lo, min(lo + cohort.BLOCK, S))]
        abunds = [(1 + rng.integers(0, 4, m.size)).astype(np.uint32) for m in mins]
        got = dev.collect(dev.launch(mins, abunds, None, sample_base=lo), timer)
        assert timer["dense_fallback_blocks"] == 0, "the bench expects compact rows throughout"
        k = int(got[0].shape[0])
        blocks.append((lo, dev.rows.clone(), dev.n_rows[1:2].clone(), dev.out[1].clone(), dev.abund_rows[2].clone(), dev.cap))
        want = matrix.cells_from_rows(got[0], k, got[2], got[4][2], lo, N)
        have = dev.matrix_cells[-1].cpu().numpy().reshape(-1).view(MATRIX_CELL_DTYPE)
        assert have.tobytes() == want.tobytes(), f"the cells of the block at {lo} differ from the numpy route's"
        print(f"block at {lo}: {k} rows, {have.size} cells, {time.perf_counter() - t_setup:.1f} s since the first", file=sys.stderr, flush=True)
    cells_d = t.cat(dev.matrix_cells)
    cells_h = cells_d.cpu().numpy().reshape(-1).view(MATRIX_CELL_DTYPE)
    n_cells = int(cells_h.size)
    d_dev = dev.dev
    block_cells = [t.zeros((cap, 3), dtype=t.int64, device=d_dev) for *_x, cap in blocks]
    block_n = t.zeros(1, dtype=t.int64, device=d_dev)
    prev_d = t.zeros((n_sets, N), dtype=t.int32, device=d_dev)
    denom_d = t.zeros((n_sets, S), dtype=t.int64, device=d_dev)

    def device_prevalence():
        db.matrix_prevalence_device(cells_d.data_ptr(), n_cells, n_sets, S, 0, prev_d.data_ptr(), denom_d.data_ptr())

    device_prevalence()
    db.synchronize()
    prev = prev_d.cpu().numpy().view(np.uint32)
    want_prev, want_denom = matrix.prevalence_numpy(cells_h, n_sets, S, None, N)
    assert np.array_equal(prev, want_prev) and np.array_equal(denom_d.cpu().numpy().view(np.uint64), want_denom), "prevalence differs"
    kept = prev[bit] >= 1
    n_kept = int(kept.sum())
    matrix.check_size(n_kept, S, True)
    row_of = matrix.row_of_ref_for(kept)
    row_of_d = t.from_numpy(row_of).to(d_dev)
    p_d = t.empty((n_kept, S), dtype=t.uint8, device=d_dev)
    m_d = t.empty((n_kept, S), dtype=t.int32, device=d_dev)
    r_d = t.empty((n_kept, S), dtype=t.float64, device=d_dev)

    def device_fill():
        db.matrix_fill_device(cells_d.data_ptr(), n_cells, bit, S, 0, row_of_d.data_ptr(), n_kept, denom_d[bit].data_ptr(), p_d.data_ptr(),
                              m_d.data_ptr(), r_d.data_ptr())

    def device_cells():
        first = len(COVS) - n_sets
        for (lo, rows, n_rows, present, med, cap), out in zip(blocks, block_cells):
            db.matrix_cells_device(rows.data_ptr(), n_rows.data_ptr(), cap, present[first].data_ptr(), n_sets, med.data_ptr(), lo,
                                   out.data_ptr(), block_n.data_ptr())

    device_fill()
    device_cells()
    db.synchronize()
    t.cuda.synchronize()
    want = matrix.fill_numpy(cells_h, bit, S, None, row_of, n_kept, want_denom[bit], True)
    assert np.array_equal(p_d.cpu().numpy(), want[0]) and np.array_equal(m_d.cpu().numpy().view(np.uint32), want[1]), "matrices differ"
    assert np.array_equal(r_d.cpu().numpy().view(np.uint64), want[2].view(np.uint64)), "relative abundances differ"
    del want

    legs = {"cells_ms": device_cells, "prevalence_ms": device_prevalence, "fill_ms": device_fill}
    times = {k: [] for k in legs}
    times["numpy_ms"] = []
    for _ in range(a.rounds):
        for k, fn in legs.items():
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            db.synchronize()
            t.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        _p, den = matrix.prevalence_numpy(cells_h, n_sets, S, None, N)
        matrix.fill_numpy(cells_h, bit, S, None, row_of, n_kept, den[bit], True)
        times["numpy_ms"].append((time.perf_counter() - t0) * 1e3)
    device_rounds = [sum(times[k][r] for k in legs) for r in range(a.rounds)]
    res = {"bench": "matrix", "n_refs": N, "samples": S, "blocks": len(blocks), "coverages": COVS, "rounds": a.rounds,
           "rows": int(sum(int(b[2].item()) for b in blocks)), "cells": n_cells, "organisms_kept": n_kept,
           "matrix_bytes": n_kept * S * 13, "check": "equal: every block's cells, prevalence counts, depth sums and the three matrices"}
    for k, v in times.items():
        res[k] = round(float(np.median(v)), 3)
        res[k.replace("_ms", "_rounds_ms")] = [round(x, 3) for x in v]
    res["device_ms"] = round(float(np.median(device_rounds)), 3)
    res["device_rounds_ms"] = [round(x, 3) for x in device_rounds]
    spread = max(max(device_rounds) - min(device_rounds), max(times["numpy_ms"]) - min(times["numpy_ms"]))
    res["margin_ms"] = round(max(0.10 * res["numpy_ms"], spread), 3)
    res["device_not_slower_than_numpy"] = bool(res["device_ms"] <= res["numpy_ms"] + res["margin_ms"])
    res["numpy_over_device"] = round(res["numpy_ms"] / max(res["device_ms"], 1e-9), 1)
    db.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
