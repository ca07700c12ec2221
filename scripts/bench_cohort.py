#!/usr/bin/env python3
"""`yacht run` over a cohort (yacht_amd/cohort.py) end to end, on a synthetic database with real-shape samples.

    python scripts/bench_cohort.py [--n-refs 85205] [--samples 1024] [--single 32] [--residual] [--abundance] [--gather --gather_top K] [--lineages [--lineages_rank RANK]] [--commit ID] [--out FILE]

Prints one JSON line: samples/s of the cohort command with its phase split (yacht_amd/cohort.py main: check, db, table,
device_setup, parse_wait, device_wait, the device time of uploads / batch counts + compact rows / presence kernel, d2h,
assemble, writes), the presence kernel alone against yh_hyp_test (host) over the same rows, and `--single` of the samples
through the single-sample command in the same process (warm) for comparison.  --residual runs the cohort (and the single
commands) with `yacht run --residual`: gpu_explain is then the phase of the residual's device work.  --abundance runs them with `yacht run --abundance`: gpu_abund is
the device time of the blocks' depth passes (YACHT_COHORT_ABUND=loop in the environment: the per-sample loop).  --gather
--gather_top K runs them with `yacht run --gather --gather_top K`: gpu_gather is the device time of the blocks' rankings
(YACHT_COHORT_GATHER=loop in the environment: the host wall time of one host-form call per sample and coverage).  --lineages
runs them with `yacht run --lineages FILE --lineages_rank RANK` over a synthetic lineage table (four consecutive organisms to
a genus, four genera to a family, and so on up): gpu_lca is the device time of the blocks' yh_lca_batch_device and rows pack
(YACHT_COHORT_LCA=loop in the environment: the HOST WALL time of one host-form yh_lca call per sample, not device time).
--matrix [--matrix_min_samples M] runs the cohort with `yacht run --matrix`: gpu_matrix is the device time of the blocks' cell
passes and of the prevalence and fill passes after the last block, matrix_files the host time of writing the tables
(YACHT_COHORT_MATRIX=host in the environment: every cell and the tables made on the host, gpu_matrix 0); the single commands
run without it.  --commit is recorded."""
from __future__ import annotations

import argparse
import json
import multiprocessing
import os
import sys
import tempfile
import time
from collections import defaultdict
from concurrent.futures import ProcessPoolExecutor
from types import SimpleNamespace

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yacht_amd import cohort, refdb_cache, run_YACHT, sigio, synth  # noqa: E402
from yacht_amd.hypothesis_recovery_src import hyp_test_native  # noqa: E402

COVS = [1, 0.5, 0.1, 0.05, 0.01]


def make_db(tmp, n_refs, seed):
    values, offsets, _ = synth.config3_like(seed=seed, n_refs=n_refs, n_sample=1000, n_present=10)
    work = os.path.join(tmp, "db_intermediate_files")
    os.makedirs(work)
    md5s = [f"{i:032x}" for i in range(n_refs)]
    sizes = np.diff(offsets).astype(np.int64)
    pd.DataFrame({"organism_name": [f"organism {i}" for i in range(n_refs)], "md5sum": md5s,
                  "num_unique_kmers_in_genome_sketch": sizes, "num_total_kmers_in_genome_sketch": sizes * 1000,
                  "genome_scale_factor": 1000}).to_csv(os.path.join(tmp, "db_manifest.tsv"), sep="\t", index=False)
    refdb_cache.save(work, md5s, 31, values, offsets)
    cfg = os.path.join(tmp, "db_config.json")
    with open(cfg, "w") as f:
        json.dump({"manifest_file_path": os.path.join(tmp, "db_manifest.tsv"), "intermediate_files_dir": work, "scale": 1000,
                   "ksize": 31, "ani_thresh": 0.95}, f)
    return cfg, values, offsets


def make_lineages(tmp, n_refs):
    """A lineage table over make_db's organisms: a species each, four consecutive ones to a genus, four genera to a family, ..."""
    path = os.path.join(tmp, "lineages.csv")
    with open(path, "w") as f:
        f.write("ident,superkingdom,phylum,class,order,family,genus,species\n")
        for i in range(n_refs):
            g = i // 4
            f.write(f"organism {i},k{g // 4096:02d},p{g // 1024:03d},c{g // 256:04d},o{g // 64:05d},f{g // 16:05d},g{g:06d},g{g:06d}s{i:06d}\n")
    return path


_REFS = None  # the references, for the sample workers (inherited by fork: this runs before anything touches the GPU)


def _one_sample(job):
    i, d, n_hashes, seed = job
    rng = np.random.default_rng(seed + i)
    mins = synth.real_shape_sample(rng, _REFS, n_sample=n_hashes)
    p = os.path.join(d, f"s{i:05d}.sig.zip")
    sigio.write_sig_zip([sigio.make_signature(mins, 31, 1000, name=f"s{i}", abundances=1 + rng.integers(0, 4, mins.size))], p)
    return p


def make_samples(tmp, values, offsets, k, n_hashes, seed, threads):
    global _REFS
    _REFS = [values[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
    d = os.path.join(tmp, "samples")
    os.makedirs(d)
    with ProcessPoolExecutor(threads, mp_context=multiprocessing.get_context("fork")) as ex:
        paths = list(ex.map(_one_sample, [(i, d, n_hashes, seed) for i in range(k)], chunksize=8))
    _REFS = None
    return paths


def kernel_vs_host(paths, cfg, threads):
    """The presence kernel and yh_hyp_test over the rows of one block (the first), every coverage."""
    import torch

    from yacht_amd import hypothesis_recovery_src as hr, utils

    conf = json.load(open(cfg))
    manifest = pd.read_csv(conf["manifest_file_path"], sep="\t")
    db = hr.get_reference_db(manifest, conf["intermediate_files_dir"], 31, threads)
    n_max = int(np.max(db.sizes))
    tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
    dev = cohort._Device(db, COVS, 31, 0.95, tab[5])
    mins = [np.asarray(utils.load_signature_with_ksize(p, 31).minhash.mins, np.uint64) for p in paths[:cohort.BLOCK]]
    b = dev.launch(mins)
    rows, pv, _, _ = dev.collect(b, defaultdict(float))
    n = rows.shape[0]
    d_rows = torch.from_numpy(rows.view(np.int32)).to(dev.dev)
    d_n = torch.tensor([n], dtype=torch.int32, device=dev.dev)
    out = dev._out(n)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev.presence(d_rows, d_n.data_ptr(), n, out)  # warm
    db.synchronize()
    reps = 5
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        dev.presence(d_rows, d_n.data_ptr(), n, out)
    ev[1].record()
    db.synchronize()
    torch.cuda.synchronize()
    ms_kernel = ev[0].elapsed_time(ev[1]) / reps
    t0 = time.perf_counter()
    host = [hyp_test_native(rows[:, 3], rows[:, 4], 31, 0.99, 0.95, c) for c in COVS]
    ms_host = (time.perf_counter() - t0) * 1e3
    got = out[0].cpu().numpy()
    worst = 0.0
    for c in range(len(COVS)):
        w = host[c][1]
        ok = ~((np.abs(got[c]) < 1e-250) & (np.abs(w) < 1e-250))
        if ok.any():
            worst = max(worst, float(np.max(np.abs(got[c][ok] - w[ok]) / np.abs(w[ok]))))
    hr.release_reference_dbs()
    return {"rows": int(n), "coverages": len(COVS), "ms_presence_kernel": round(ms_kernel, 3), "ms_yh_hyp_test_host": round(ms_host, 1),
            "rows_x_covs_per_s_kernel": round(n * len(COVS) / (ms_kernel / 1e3)), "rows_x_covs_per_s_host": round(n * len(COVS) / (ms_host / 1e3)),
            "p_val_max_rel_diff_kernel_vs_host": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--sample-hashes", type=int, default=83_000)
    ap.add_argument("--single", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1002)
    ap.add_argument("--residual", action="store_true")
    ap.add_argument("--abundance", action="store_true")
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--gather_top", type=int, default=None)
    ap.add_argument("--lineages", action="store_true")
    ap.add_argument("--lineages_rank", default="genus")
    ap.add_argument("--matrix", action="store_true")
    ap.add_argument("--matrix_min_samples", type=int, default=None)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="bench_cohort_")
    t0 = time.perf_counter()
    cfg, values, offsets = make_db(tmp, a.n_refs, a.seed)
    paths = make_samples(tmp, values, offsets, a.samples, a.sample_hashes, a.seed, a.threads)
    setup_s = time.perf_counter() - t0
    del values, offsets

    out = os.path.join(tmp, "cohort_out")
    os.makedirs(out)
    args = SimpleNamespace(json=cfg, sample_file=paths, significance=0.99, num_threads=a.threads, keep_raw=False, show_all=False,
                           min_coverage_list=COVS, outdir=out, residual=a.residual, residual_coverage=None,
                           abundance=a.abundance, gather=a.gather, gather_top=a.gather_top, gather_min_hits=1, gather_coverage=None,
                           lineages=make_lineages(tmp, a.n_refs) if a.lineages else None,
                           lineages_rank=a.lineages_rank if a.lineages else None,
                           matrix=a.matrix, matrix_coverage=None, matrix_min_samples=a.matrix_min_samples)
    t0 = time.perf_counter()
    phases = cohort.main(args, paths)
    wall = time.perf_counter() - t0
    summ = pd.read_csv(os.path.join(out, "results", "cohort_samples.tsv"), sep="\t")

    kern = kernel_vs_host(paths, cfg, a.threads)

    single_s = []
    for i, p in enumerate(paths[:a.single]):
        od = os.path.join(tmp, f"single_{i}")
        os.makedirs(od)
        t0 = time.perf_counter()
        run_YACHT.main(SimpleNamespace(**{**vars(args), "sample_file": p, "outdir": od, "matrix": False, "matrix_min_samples": None}))
        single_s.append(time.perf_counter() - t0)
    from yacht_amd import hypothesis_recovery_src as hr

    hr.release_reference_dbs()
    res = {
        "workload": f"synthetic database of {a.n_refs} references (config3_like), {a.samples} real-shape samples of "
                    f"~{a.sample_hashes} hashes as .sig.zip, coverages {COVS}",
        "commit": a.commit,
        "residual": bool(a.residual),
        "abundance": bool(a.abundance),
        "cohort_abund": os.environ.get("YACHT_COHORT_ABUND", ""),
        "gather": bool(a.gather),
        "gather_top": a.gather_top,
        "cohort_gather": os.environ.get("YACHT_COHORT_GATHER", ""),
        "lineages": bool(a.lineages),
        "lineages_rank": a.lineages_rank if a.lineages else None,
        "cohort_lca": os.environ.get("YACHT_COHORT_LCA", ""),
        "matrix": bool(a.matrix),
        "matrix_min_samples": a.matrix_min_samples,
        "cohort_matrix": os.environ.get("YACHT_COHORT_MATRIX", ""),
        "setup_s": round(setup_s, 1),
        "bottleneck": None,
        "cohort": {"samples": a.samples, "wall_s": round(wall, 2), "samples_per_s": round(a.samples / wall, 2),
                   "presence_rows": int(sum(1 for _ in open(os.path.join(out, "results", "cohort_presence.tsv"))) - 1),
                   "phases_s": {k: round(v, 3) for k, v in phases.items()},
                   "rows_per_sample_mean": round(float(summ["n_overlapping"].mean()), 1),
                   "no_overlap": int((summ["status"] == "no_overlap").sum())},
        "presence_kernel_vs_yh_hyp_test": kern,
        "single_command": {"samples": len(single_s), "mean_s": round(float(np.mean(single_s)), 3) if single_s else None,
                           "first_s": round(single_s[0], 3) if single_s else None,
                           "samples_per_s_warm": round(len(single_s[1:]) / sum(single_s[1:]), 2) if len(single_s) > 1 else None},
    }
    host_phases = {k: v for k, v in phases.items() if k not in ("total", "dense_fallback_blocks", "lca_repacked_blocks") and not k.startswith("gpu_")}
    res["bottleneck"] = max(host_phases, key=host_phases.get)
    if single_s:
        res["cohort_speedup_vs_single_warm"] = round(res["cohort"]["samples_per_s"] / max(res["single_command"]["samples_per_s_warm"] or 1e-9, 1e-9), 2)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
