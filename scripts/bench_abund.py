#!/usr/bin/env python3
"""Device time of the abundance pass (yh_abund_device) next to the indexed run step it rides on.

    python scripts/bench_abund.py [--n-refs 85205] [--iters 200] [--warmup 30] [--rounds 3] [--out FILE]

On the synthetic database at GTDB rs214 scale (synth.config3_device) and for two sample shapes -- a 10^6-hash sample and a
real-shape 83 k-hash sample (synth.sample_device) -- three calls are timed in the same process, on the same samples:
yh_abund_device with the median, yh_abund_device without it (d_med_match = NULL: no hit list, no sort), and
yh_run_indexed_device as the yardstick.  HIP events on the handle's stream around `iters` back-to-back calls that rotate
through eight samples (so the buckets come from HBM, not from a cache warmed by the previous call), after a warm-up of
every call; the three calls alternate inside each of `rounds` rounds and the median round is reported with the spread.
Prints one JSON line and writes it to --out (default profiles/abund/bench_abund.json).  Also records what parsing the
per-hash abundances of a 10^6-hash sample file costs on the host (the general reader: abundance.sample_abundances).

    python scripts/bench_abund.py --batch [--batch-iters 5] [--batch-warmup 2] [--rounds 3] [--out FILE]

times the block form instead: ONE yh_abund_batch_device against a loop of yh_abund_device over the same resident block, in
the same process, with the median and sums-only, for a block of 256 real-shape 83 k-hash samples and one of 32 samples of
10^6 hashes.  HIP events around `batch-iters` passes over the block; the four calls alternate inside each round; per sample
microseconds, the median round with every round beside it (default --out: profiles/abund/bench_abund_batch.json).  The
loop's time holds what the loop costs as the cohort runs it: where the host cannot queue the per-sample calls as fast as the
device finishes them, the stream waits for the host."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yacht_amd import _lib, abundance, sigio, synth, utils  # noqa: E402
from yacht_amd.engine import RefDB  # noqa: E402

N_ROTATE = 8


def parse_cost(n_hashes: int) -> dict:
    """Host seconds to get the per-hash abundances of an n-hash sample archive next to the native read of its hashes."""
    rng = np.random.default_rng(77)
    mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), n_hashes, dtype=np.uint64))
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.sig.zip")
        sigio.write_sig_zip([sigio.make_signature(mins, 31, 1000, name="s", abundances=1 + rng.integers(0, 9, mins.size))], p)
        t0 = time.perf_counter()
        sig = utils.load_signature_with_ksize(p, 31)
        t1 = time.perf_counter()
        ab = abundance.sample_abundances(sig, p)
        t2 = time.perf_counter()
        assert ab.size == mins.size
    return {"n_hashes": int(mins.size), "load_signature_s": round(t1 - t0, 4), "abundances_s": round(t2 - t1, 4)}


def bench_batch(args, torch, db, values, offsets, N: int, stream, result: dict) -> None:
    """One yh_abund_batch_device against the loop of yh_abund_device over the same resident block."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    for name, shape, n_sample, b in (("256x_real_shape_83k", "real", 83_000, 256), ("32x_1e6_hash", "present", 1_000_000, 32)):
        samples = [synth.sample_device(values, offsets, seed=1900 + i, n_sample=n_sample, shape=shape) for i in range(b)]
        offs = np.zeros(b + 1, dtype=np.int64)
        offs[1:] = np.cumsum([int(s.numel()) for s in samples])
        total = int(offs[-1])
        d_s = torch.cat(samples)
        del samples
        d_o = torch.from_numpy(offs).to(dev)
        d_a = torch.randint(1, 1001, (total,), generator=g, device=dev, dtype=torch.int32)
        out = [(torch.zeros((b, N), dtype=torch.int64, device=dev), torch.zeros((b, N), dtype=torch.int64, device=dev),
                torch.zeros((b, N), dtype=torch.float64, device=dev)) for _ in range(2)]
        torch.cuda.synchronize()

        def batched(o, med=True):
            db.abundance_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), b, total, o[0].data_ptr(), o[1].data_ptr(),
                                      o[2].data_ptr() if med else 0)

        def looped(o, med=True):
            for s in range(b):
                db.abundance_device(d_s.data_ptr() + 8 * int(offs[s]), d_a.data_ptr() + 4 * int(offs[s]), int(offs[s + 1] - offs[s]),
                                    o[0][s].data_ptr(), o[1][s].data_ptr(), o[2][s].data_ptr() if med else 0)

        # what the timed calls compute, once, against each other: the contract is bit-identical rows
        batched(out[0])
        looped(out[1])
        db.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out[0], out[1])), "the batched rows differ from the per-sample loop's"
        calls = (("batched_with_median", lambda: batched(out[0])), ("looped_with_median", lambda: looped(out[1])),
                 ("batched_sums_only", lambda: batched(out[0], False)), ("looped_sums_only", lambda: looped(out[1], False)))
        times = {k: [] for k, _ in calls}
        with torch.cuda.stream(stream):
            for _k, fn in calls:
                for _ in range(args.batch_warmup):
                    fn()
            db.synchronize()
            for _ in range(args.rounds):
                for k, fn in calls:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _i in range(args.batch_iters):
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / args.batch_iters / b)
        shape_out = {"n_samples": b, "total_hashes": total, "pairs_with_a_median": int((out[0][2] > 0).sum())}
        for k, v in times.items():
            shape_out[k + "_us_per_sample"] = round(float(np.median(v)), 2)
            shape_out[k + "_rounds_us_per_sample"] = [round(x, 2) for x in v]
        for kind in ("with_median", "sums_only"):
            bt, lp = times["batched_" + kind], times["looped_" + kind]
            shape_out[kind + "_looped_over_batched"] = round(float(np.median(lp)) / float(np.median(bt)), 2)
            shape_out[kind + "_batched_faster_outside_the_spread"] = bool(max(bt) < min(lp))
        result["shapes"][name] = shape_out
        del d_s, d_a, out
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", action="store_true", help="time yh_abund_batch_device against a loop of yh_abund_device")
    ap.add_argument("--batch-iters", type=int, default=5)
    ap.add_argument("--batch-warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "abund",
                                "bench_abund_batch.json" if args.batch else "bench_abund.json")
    import torch

    assert _lib.device_count() >= 1, "bench_abund.py needs an MI355X"
    dev = torch.device("cuda:0")
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=args.n_refs, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    N = args.n_refs
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    result = {"bench": "abund", "n_refs": N, "n_hashes_db": int(values.numel()), "iters": args.iters, "warmup": args.warmup,
              "rounds": args.rounds, "samples_rotated": N_ROTATE, "info": {k: int(v) for k, v in db.info().items()}, "shapes": {}}
    if args.batch:
        result.update({"bench": "abund_batch", "iters": args.batch_iters, "warmup": args.batch_warmup, "tile": _lib.YH_ABUND_BATCH_TILE})
        del result["samples_rotated"]
        bench_batch(args, torch, db, values, offsets, N, stream, result)
    for name, shape, n_sample in () if args.batch else (("1e6_hash", "present", 1_000_000), ("real_shape_83k", "real", 83_000)):
        samples = [synth.sample_device(values, offsets, seed=900 + i, n_sample=n_sample, shape=shape) for i in range(N_ROTATE)]
        abunds = [torch.randint(1, 1001, (int(s.numel()),), generator=g, device=dev, dtype=torch.int32) for s in samples]
        w_ov = torch.zeros(N, dtype=torch.int64, device=dev)
        w_m = torch.zeros(N, dtype=torch.int64, device=dev)
        med = torch.zeros(N, dtype=torch.float64, device=dev)
        cnt = [torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(3)]
        torch.cuda.synchronize()

        def abund_med(i):
            db.abundance_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), w_ov.data_ptr(), w_m.data_ptr(),
                                med.data_ptr())

        def abund_sums(i):
            db.abundance_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), w_ov.data_ptr(), w_m.data_ptr(), 0)

        def run_indexed(i):
            db.run_indexed_device(samples[i].data_ptr(), int(samples[i].numel()), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())

        calls = (("abund_with_median_us", abund_med), ("abund_sums_only_us", abund_sums), ("run_indexed_us", run_indexed))
        # the results the timed calls produce, once, against each other: the sums with and without the median are the same
        abund_med(0)
        db.synchronize()
        a0, a1 = w_ov.clone(), w_m.clone()
        abund_sums(0)
        run_indexed(0)
        db.synchronize()
        assert torch.equal(a0, w_ov) and torch.equal(a1, w_m)
        hits = int((cnt[0] > 0).sum())
        times = {k: [] for k, _ in calls}
        with torch.cuda.stream(stream):
            for _k, fn in calls:
                for i in range(args.warmup):
                    fn(i % N_ROTATE)
            db.synchronize()
            for _ in range(args.rounds):
                for k, fn in calls:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for i in range(args.iters):
                        fn(i % N_ROTATE)
                    e1.record(stream)
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        shape_out = {"n_sample": int(samples[0].numel()), "references_overlapping": hits,
                     "single_holder_hits": int(db.run_counts(samples[0].cpu().numpy().view(np.uint64))[2].sum())}
        for k, v in times.items():
            shape_out[k] = round(float(np.median(v)), 2)
            shape_out[k.replace("_us", "_rounds_us")] = [round(x, 2) for x in v]
        shape_out["sums_only_over_run_indexed"] = round(shape_out["abund_sums_only_us"] / shape_out["run_indexed_us"], 3)
        shape_out["with_median_over_run_indexed"] = round(shape_out["abund_with_median_us"] / shape_out["run_indexed_us"], 3)
        result["shapes"][name] = shape_out
    db.close()
    if not args.batch:
        result["host_parse_1e6"] = parse_cost(1_000_000)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
