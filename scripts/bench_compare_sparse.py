#!/usr/bin/env python3
"""The two routes of the compare pass side by side: yh_compare_device (dense tiles) and yh_compare_sparse_device (through
the shared hashes), on the standard shapes of scripts/bench_compare.py and on a sweep that moves the number of cell updates.

    python scripts/bench_compare_sparse.py [--shapes 256x83k 1024x83k 32x1M] [--sweep] [--parent-lib PATH] [--rounds 3]
                                           [--no-baseline] [--commit ID] [--out FILE] [--fit FILE]

Per point (a shape, or a sweep point):
  check      cells of a subset of pairs equal the numpy oracle (bench_compare.oracle_pairs) on BOTH routes, and the two
             routes' whole matrices and self rows are equal, before anything is timed
  dense      one symmetric yh_compare_device; with --parent-lib also the same call into the parent commit's library, the two
             alternating round by round: the dense figure the new route is held against is the parent's
  sparse     one symmetric yh_compare_sparse_device, hash_bits from the data
  estimator  what route auto pays before it chooses: yh_compare_sparse_count_device (records, sort, runs) over the samples'
             prefixes below 2^(hash_bits - YH_COMPARE_SAMPLE_LOG2), packed as a set of their own, and the read-back of its
             figure pairs_sampled
  auto       the route yh_compare_routed(auto) takes on the same samples (host form, once, untimed: its uploads would
             swamp the figure) and estimator + that route's time
  HIP events, one warm call, then the median of --rounds rounds with min and max.
--sweep: 256 samples of 83 000 uniform hashes of which a fraction f comes from a core common to all, f in 0, 0.01, 0.1,
0.5, 0.9, and 32 samples of 10^6 at f in 0, 0.5; per point T, P, D and both times go to --fit with the least-squares
constants of  sparse = c0 + c1 T + c2 P  and  dense = d0 + d1 D  (nanoseconds; relative errors, no constant below zero).
--no-baseline skips the earlier n_shared-only route (a database of the samples, the samples run against it), which
bench_compare.py measures.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_compare as bc  # noqa: E402

from yacht_amd import _lib, compare, synth  # noqa: E402

SWEEP = [(256, 83_000, f) for f in (0.0, 0.01, 0.1, 0.5, 0.9)] + [(32, 1_000_000, f) for f in (0.0, 0.5)]
TOP = 1 << 54  # (a sketch of scaled = 1000 fills about 2^54 of the hash space)


def draw_core(torch, n, n_hashes, f, seed):
    """n samples of about n_hashes uniform hashes below TOP, of which a fraction f is one core common to all."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n_core = int(round(f * n_hashes))
    core = torch.randint(0, TOP, (n_core,), generator=g, device="cuda", dtype=torch.int64)
    parts = [torch.unique(torch.cat([core, torch.randint(0, TOP, (n_hashes - n_core,), generator=g, device="cuda", dtype=torch.int64)]))
             for _ in range(n)]
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum([int(p.numel()) for p in parts])
    cat = torch.cat(parts).contiguous()
    ab = torch.randint(1, 5, (int(offs[-1]),), generator=g, device="cuda", dtype=torch.int32)
    return cat, torch.from_numpy(offs).cuda(), offs, ab


def parent_library(path):
    lib = C.CDLL(path)
    for name in ("yh_compare_work_bytes", "yh_compare_device"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def timed(torch, call, rounds):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(rounds):
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return ms


def margin_of(*spreads):
    return max([0.10] + [(s["max_ms"] - s["min_ms"]) / s["median_ms"] for s in spreads])


def bench_point(torch, name, cat, d_offs, offs, ab, rounds, seed, parent, baseline_ms=None):
    n, total = offs.size - 1, int(offs[-1])
    dev = cat.device
    bits = max(1, int(cat.max().item()).bit_length())
    cells = [torch.empty((n, n, 4), dtype=torch.int64, device=dev) for _ in range(2)]
    selfs = [torch.empty((n, 4), dtype=torch.int64, device=dev) for _ in range(2)]
    need = max(compare.work_bytes(n, n, total, total), compare.sparse_work_bytes(n, n, total, total))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(7, dtype=torch.int64, device=dev)
    v = C.c_void_p

    def dense():
        compare.compare_device(cat.data_ptr(), d_offs.data_ptr(), ab.data_ptr(), 0, n, total, cat.data_ptr(), d_offs.data_ptr(), ab.data_ptr(), 0,
                               n, total, 0, 0, cells[0].data_ptr(), n, selfs[0].data_ptr(), selfs[0].data_ptr(), work.data_ptr(), work.numel(), 0)

    def dense_parent():
        rc = parent.yh_compare_device(v(cat.data_ptr()), v(d_offs.data_ptr()), v(ab.data_ptr()), v(0), n, total, v(cat.data_ptr()),
                                      v(d_offs.data_ptr()), v(ab.data_ptr()), v(0), n, total, 0, 0, v(cells[0].data_ptr()), n,
                                      v(selfs[0].data_ptr()), v(selfs[0].data_ptr()), v(work.data_ptr()), work.numel(), v(0))
        assert rc == 0, rc

    def sparse():
        compare.compare_sparse_device(cat.data_ptr(), d_offs.data_ptr(), ab.data_ptr(), 0, n, total, cat.data_ptr(), d_offs.data_ptr(),
                                      ab.data_ptr(), 0, n, total, 0, 0, cells[1].data_ptr(), n, selfs[1].data_ptr(), selfs[1].data_ptr(),
                                      work.data_ptr(), work.numel(), 0, bits, d_info.data_ptr())

    # the samples' prefixes below the estimator's window, packed as a set of their own
    window = 1 << max(bits - _lib.YH_COMPARE_SAMPLE_LOG2, 0)
    mask = cat < window
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(mask, 0)])
    p_offs = csum[d_offs].contiguous()
    p_cat, p_total = cat[mask].contiguous(), int(csum[-1].item())
    p_info = torch.zeros(7, dtype=torch.int64, device=dev)

    def estimator():
        compare.sparse_count_device(p_cat.data_ptr(), p_offs.data_ptr(), 0, n, p_total, p_cat.data_ptr(), p_offs.data_ptr(), 0, n, p_total, 0, 0,
                                    work.data_ptr(), work.numel(), 0, max(bits - _lib.YH_COMPARE_SAMPLE_LOG2, 1), p_info.data_ptr())
        p_info[2].item()  # (the read-back of the pair count: the events around this call see it)

    estimator()
    dense()
    sparse()
    torch.cuda.synchronize()
    got = [c.cpu().numpy().view(np.uint64) for c in cells]
    assert np.array_equal(got[0], got[1]), (name, "the two routes' cells differ")
    assert np.array_equal(selfs[0].cpu().numpy(), selfs[1].cpu().numpy()), (name, "the two routes' self rows differ")
    rng = np.random.default_rng(seed)
    pairs = [(0, 0), (0, n - 1), (n - 1, n - 1)] + [tuple(int(x) for x in rng.integers(0, n, 2)) for _ in range(5)]
    for (i, j), (n_sh, mn, dot) in bc.oracle_pairs(cat, offs, ab, pairs).items():
        want = (n_sh, mn, dot & (2 ** 64 - 1), dot >> 64)
        for g in got:
            assert tuple(int(x) for x in g[i, j]) == want == tuple(int(x) for x in g[j, i]), (name, i, j, g[i, j], want)
    info = [int(x) for x in d_info.cpu().numpy().view(np.uint64)]
    res = {"samples": n, "hashes": total, "hash_bits": bits, "checked_pairs": len(pairs), "T": info[0], "shared_hashes": info[1], "P": info[2],
           "longest_run": info[3], "D": info[4], "pairs_sampled": int(p_info.cpu().numpy().view(np.uint64)[2]), "window_entries": p_total}
    assert res["P"] == int(np.triu(got[0][..., 0].astype(object), 1).sum()), (name, "P is not the shared hashes of the pairs")
    del got
    ms = {"dense": [], "dense_parent": [], "sparse": [], "estimator": []}
    for _ in range(rounds):  # the routes alternate round by round
        if parent is not None:
            ms["dense_parent"] += timed(torch, dense_parent, 1)
        ms["dense"] += timed(torch, dense, 1)
        ms["sparse"] += timed(torch, sparse, 1)
        ms["estimator"] += timed(torch, estimator, 1)
    for k, vals in ms.items():
        if vals:
            res[k] = bc.spread(vals)
    # the route auto takes on these samples: the host form, once, not timed
    host = (cat.cpu().numpy().view(np.uint64), offs.astype(np.uint64), ab.cpu().numpy().view(np.uint32), None)
    auto = compare.compare_packed(host, None, route="auto")
    del host
    res["auto_route"], res["auto_pairs_sampled"], res["auto_estimated"] = auto.info["route"], auto.info["pairs_sampled"], auto.info["estimated"]
    assert auto.info["pairs_sampled"] == res["pairs_sampled"], (name, auto.info, res["pairs_sampled"])
    del auto
    ref = res.get("dense_parent", res["dense"])
    chosen = res["dense"] if res["auto_route"] == "dense" else res["sparse"]
    res["auto_ms"] = round(res["estimator"]["median_ms"] + chosen["median_ms"], 3)
    best = min(ref["median_ms"], res["sparse"]["median_ms"])
    m = margin_of(ref, res["sparse"], res["estimator"])
    res["margin"] = round(m, 3)
    res["sparse_vs_parent_dense"] = round(ref["median_ms"] / res["sparse"]["median_ms"], 3)
    res["auto_vs_best_forced"] = round(res["auto_ms"] / best, 3)
    res["auto_no_slower_than_best"] = bool(res["auto_ms"] <= best * (1 + m))
    if baseline_ms is not None:
        res["earlier_route_ms"] = baseline_ms
        res["auto_vs_earlier_route"] = round(res["auto_ms"] / baseline_ms, 3)
        res["auto_no_slower_than_earlier_route"] = bool(res["auto_ms"] <= baseline_ms * (1 + m))
    return res


def _nonneg_lstsq(rows, times):
    """Least squares on RELATIVE errors (every point weighs the same, whatever its time) with no constant below zero: the
    best of the fits over every subset of the constants, the others held at zero."""
    rows, times = np.asarray(rows, dtype=np.float64), np.asarray(times, dtype=np.float64)
    best = None
    for subset in range(1, 1 << rows.shape[1]):
        cols = [k for k in range(rows.shape[1]) if subset >> k & 1]
        sol, *_ = np.linalg.lstsq(rows[:, cols] / times[:, None], np.ones(times.size), rcond=None)
        if (sol < 0).any():
            continue
        full = np.zeros(rows.shape[1])
        full[cols] = sol
        err = float((((rows @ full) / times - 1.0) ** 2).sum())
        if best is None or err < best[0]:
            best = (err, full)
    return [float(x) for x in best[1]]


def fit(points):
    """In nanoseconds: sparse = c0 + c1 T + c2 P, dense = d0 + d1 D (the parent's dense time where it was taken)."""
    c = _nonneg_lstsq([[1.0, p["T"], p["P"]] for p in points], [p["sparse"]["median_ms"] * 1e6 for p in points])
    d = _nonneg_lstsq([[1.0, p["D"]] for p in points], [p.get("dense_parent", p["dense"])["median_ms"] * 1e6 for p in points])
    return c, d


def write_fit(path, points, names, c, d, commit):
    lines = [f"# sweep of scripts/bench_compare_sparse.py, commit {commit}; one MI355X; times are medians in ms",
             "# point                  T            P               D         sparse_ms   dense_ms  model_sparse  model_dense  auto"]
    for name, p in zip(names, points):
        dm = p.get("dense_parent", p["dense"])["median_ms"]
        lines.append(f"{name:<18} {p['T']:>12} {p['P']:>12} {p['D']:>15} {p['sparse']['median_ms']:>12.3f} {dm:>10.3f} "
                     f"{(c[0] + c[1] * p['T'] + c[2] * p['P']) / 1e6:>13.3f} {(d[0] + d[1] * p['D']) / 1e6:>12.3f}  {p['auto_route']}")
    lines += ["", "least squares on relative errors, no constant below zero, nanoseconds:", f"sparse = c0 + c1 * T + c2 * P   c0 = {c[0]:.6g}  c1 = {c[1]:.6g}  c2 = {c[2]:.6g}",
              f"dense  = d0 + d1 * D            d0 = {d[0]:.6g}  d1 = {d[1]:.6g}", ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(bc.SHAPES), choices=list(bc.SHAPES))
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1002)
    ap.add_argument("--parent-lib", default=None, help="libyacht_hip.so of the parent commit: its dense pass is the yardstick")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fit", default=None)
    args = ap.parse_args()
    import torch

    assert _lib.device_count() >= 1, "bench_compare_sparse needs the device"
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    out = {"workload": "symmetric calls of yh_compare_device and yh_compare_sparse_device on the same samples, abundances 1..4",
           "commit": args.commit, "dense_yardstick": "parent commit's library" if parent is not None else "this library",
           "run_small": _lib.YH_COMPARE_RUN_SMALL, "chunk": _lib.YH_COMPARE_SPARSE_CHUNK, "sample_log2": _lib.YH_COMPARE_SAMPLE_LOG2,
           "shapes": {}, "sweep": {}}
    if args.shapes:
        values, offsets, _ = synth.config3_device(seed=args.seed, n_refs=args.n_refs, n_sample=1000, n_present=10)
        drawn = {}
        for n_hashes in sorted({bc.SHAPES[name][1] for name in args.shapes}):
            n = max(bc.SHAPES[name][0] for name in args.shapes if bc.SHAPES[name][1] == n_hashes)
            drawn[n_hashes] = bc.draw(torch, values, offsets, n, n_hashes, args.seed)
        del values, offsets
        for name in args.shapes:
            n, n_hashes = bc.SHAPES[name]
            cat, d_offs, offs, ab = drawn[n_hashes]
            offs, d_offs = offs[:n + 1], d_offs[:n + 1].contiguous()
            total = int(offs[-1])
            baseline_ms = None
            if not args.no_baseline:
                got = bc.bench_shape(torch, drawn, name, args.rounds, args.seed, True).get("baseline")
                baseline_ms = got["median_ms"] if isinstance(got, dict) else None
            out["shapes"][name] = bench_point(torch, name, cat[:total], d_offs, offs, ab[:total], args.rounds, args.seed, parent, baseline_ms)
            print(name, json.dumps(out["shapes"][name]), file=sys.stderr, flush=True)
        del drawn
    if args.sweep:
        names = []
        for n, n_hashes, f in SWEEP:
            name = f"{n}x{n_hashes // 1000}k_f{f:g}"
            cat, d_offs, offs, ab = draw_core(torch, n, n_hashes, f, args.seed)
            out["sweep"][name] = bench_point(torch, name, cat, d_offs, offs, ab, args.rounds, args.seed, parent)
            names.append(name)
            print(name, json.dumps(out["sweep"][name]), file=sys.stderr, flush=True)
            del cat, d_offs, ab
        c, d = fit([out["sweep"][k] for k in names])
        if args.fit:  # (a run that does not write the fit reports the library's constants at work, not a fit of its own)
            out["fit_ns"] = {"c0": c[0], "c1": c[1], "c2": c[2], "d0": d[0], "d1": d[1]}
            write_fit(args.fit, [out["sweep"][k] for k in names], names, c, d, args.commit)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
