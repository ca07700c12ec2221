#!/usr/bin/env python3
"""The compare pass (yh_compare_device) on the project's standard shapes, against the route that existed before it.

    python scripts/bench_compare.py [--shapes 256x83k 1024x83k 32x1M] [--n-refs 85205] [--rounds 3] [--no-baseline] [--commit ID] [--out FILE]

Samples are drawn as scripts/bench_cohort.py draws them -- real-shape samples of a config3 database (synth.sample_device,
shape="real") -- directly in HBM, with abundances 1..4.  Per shape:
  check     cells and self rows of a subset of pairs equal the numpy oracle (np.intersect1d, Python ints), before any timing
  compare   one symmetric yh_compare_device over all samples: all three sums of every pair.  HIP events, one warm call, then
            the median of --rounds rounds with their spread (min, max)
  baseline  what gives n_shared alone without this pass: one yh_db_create_device on the same samples plus
            yh_run_batch_device of them against it in blocks of 256, build included, between the same events; when the
            route cannot run a shape (memory, the side list), its error is recorded in place of a time
  rate      the one-touch bytes (total_a + total_b) x 12 B over the compare time, for orientation
  verdict   compare no slower than the baseline, within 10 % or the rounds' spread, whichever is larger
Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yacht_amd import _lib, compare, synth  # noqa: E402
from yacht_amd.engine import RefDB  # noqa: E402

SHAPES = {"256x83k": (256, 83_000), "1024x83k": (1024, 83_000), "32x1M": (32, 1_000_000)}
BLOCK = _lib.YH_BATCH_MAX_SAMPLES


def draw(torch, values, offsets, n, n_hashes, seed):
    """n samples back to back in HBM: (hashes int64, offsets int64 [n + 1] on the device and on the host, abundances int32)."""
    parts = [synth.sample_device(values, offsets, seed=seed + i, n_sample=n_hashes, shape="real") for i in range(n)]
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum([int(p.numel()) for p in parts])
    cat = torch.cat(parts).contiguous()
    g = torch.Generator(device=cat.device)
    g.manual_seed(seed)
    ab = torch.randint(1, 5, (int(offs[-1]),), generator=g, device=cat.device, dtype=torch.int32)
    return cat, torch.from_numpy(offs).to(cat.device), offs, ab


def oracle_pairs(cat, offs, ab, pairs):
    out = {}
    for i, j in pairs:
        xa, xb = (cat[int(offs[s]):int(offs[s + 1])].cpu().numpy().view(np.uint64) for s in (i, j))
        aa, bb = (ab[int(offs[s]):int(offs[s + 1])].cpu().numpy().astype(np.int64) for s in (i, j))
        _, ia, ib = np.intersect1d(xa, xb, assume_unique=True, return_indices=True)
        u, v = [int(t) for t in aa[ia]], [int(t) for t in bb[ib]]
        out[(i, j)] = (len(u), sum(min(p, q) for p, q in zip(u, v)), sum(p * q for p, q in zip(u, v)))
    return out


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "rounds": len(ms)}


def bench_shape(torch, drawn, name, rounds, seed, baseline):
    n, n_hashes = SHAPES[name]
    cat, d_offs, offs, ab = drawn[n_hashes]  # (the first n samples of the largest shape of this sample size)
    offs, d_offs = offs[:n + 1], d_offs[:n + 1].contiguous()
    total = int(offs[-1])
    cat, ab = cat[:total], ab[:total]
    dev = cat.device
    cells = torch.empty((n, n, 4), dtype=torch.int64, device=dev)
    selfs = torch.empty((n, 4), dtype=torch.int64, device=dev)
    work = torch.empty(compare.work_bytes(n, n, total, total), dtype=torch.uint8, device=dev)

    def call():
        compare.compare_device(cat.data_ptr(), d_offs.data_ptr(), ab.data_ptr(), 0, n, total, cat.data_ptr(), d_offs.data_ptr(), ab.data_ptr(), 0,
                               n, total, 0, 0, cells.data_ptr(), n, selfs.data_ptr(), selfs.data_ptr(), work.data_ptr(), work.numel(), 0)

    call()  # warm, and the check
    torch.cuda.synchronize()
    got = cells.cpu().numpy().view(np.uint64)
    rng = np.random.default_rng(seed)
    pairs = [(0, 0), (0, n - 1), (n - 1, n - 1)] + [tuple(int(x) for x in rng.integers(0, n, 2)) for _ in range(9)]
    for (i, j), (n_sh, mn, dot) in oracle_pairs(cat, offs, ab, pairs).items():
        want = (n_sh, mn, dot & (2 ** 64 - 1), dot >> 64)
        assert tuple(int(x) for x in got[i, j]) == want == tuple(int(x) for x in got[j, i]), (name, i, j, got[i, j], want)
    got_self = selfs.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_self[:, 0], np.diff(offs).astype(np.uint64)) and np.array_equal(got[np.arange(n), np.arange(n)], got_self)
    res = {"samples": n, "hashes": total, "checked_pairs": len(pairs), "mean_shared_per_pair": round(float(got[..., 0].sum() - got_self[:, 0].sum()) / max(n * n - n, 1), 1)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(rounds):
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    res["compare"] = spread(ms)
    res["one_touch_GBps"] = round(2 * total * 12 / (res["compare"]["median_ms"] * 1e6), 2)
    if not baseline:
        res["baseline"] = "unmeasured"
        return res
    try:  # n_shared alone: a database of the samples, the samples against it in blocks of 256, build included
        counts = torch.zeros((3, BLOCK, n), dtype=torch.int32, device=dev)
        rebased = [(d_offs[b0:min(b0 + BLOCK, n) + 1] - d_offs[b0]).contiguous() for b0 in range(0, n, BLOCK)]
        ms = []
        for r in range(rounds + 1):
            ev[0].record()
            db = RefDB.from_device(cat.data_ptr(), d_offs.data_ptr(), n, device=dev.index or 0)
            try:
                for k, b0 in enumerate(range(0, n, BLOCK)):
                    b = min(BLOCK, n - b0)
                    db.run_batch_device(cat.data_ptr() + 8 * int(offs[b0]), rebased[k].data_ptr(), b, int(offs[b0 + b] - offs[b0]),
                                        counts[0].data_ptr(), counts[1].data_ptr(), counts[2].data_ptr())
                db.synchronize()
                ev[1].record()
                torch.cuda.synchronize()
                if r == 0:  # (warm round) the last block's overlap counts are the compare pass's n_shared
                    want = got[b0:b0 + b, :, 0].astype(np.int64)
                    assert np.array_equal(counts[0, :b].cpu().numpy().astype(np.int64), want), "baseline overlap differs from n_shared"
                else:
                    ms.append(ev[0].elapsed_time(ev[1]))
            finally:
                db.close()
        res["baseline"] = spread(ms)
        ratio = res["baseline"]["median_ms"] / res["compare"]["median_ms"]
        margin = max(0.10, (res["compare"]["max_ms"] - res["compare"]["min_ms"]) / res["compare"]["median_ms"],
                     (res["baseline"]["max_ms"] - res["baseline"]["min_ms"]) / res["baseline"]["median_ms"])
        res["baseline_over_compare"] = round(ratio, 3)
        res["margin"] = round(margin, 3)
        res["verdict"] = "faster" if ratio > 1 + margin else "no slower (within the margin)" if ratio >= 1 - margin else "slower"
    except (_lib.YachtHipError, RuntimeError) as e:
        res["baseline"] = f"cannot run this shape: {e}"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1002)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert _lib.device_count() >= 1, "bench_compare needs the device"
    values, offsets, _ = synth.config3_device(seed=args.seed, n_refs=args.n_refs, n_sample=1000, n_present=10)
    out = {"workload": f"real-shape samples of a synthetic database of {args.n_refs} references (synth.config3_device), abundances 1..4, "
                       "one symmetric yh_compare_device per shape", "commit": args.commit, "tile": _lib.YH_COMPARE_TILE,
           "slice": _lib.YH_COMPARE_SLICE, "shapes": {}}
    drawn = {}
    for n_hashes in sorted({SHAPES[name][1] for name in args.shapes}):
        n = max(SHAPES[name][0] for name in args.shapes if SHAPES[name][1] == n_hashes)
        drawn[n_hashes] = draw(torch, values, offsets, n, n_hashes, args.seed)
    del values, offsets
    for name in args.shapes:
        out["shapes"][name] = bench_shape(torch, drawn, name, args.rounds, args.seed, not args.no_baseline)
        print(name, json.dumps(out["shapes"][name]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
