#!/usr/bin/env python3
"""Device time of the per-sample-hash pass (yh_explain_device) next to the passes that make the same reads.

    python scripts/bench_explain.py [--n-refs 85205] [--iters 200] [--warmup 30] [--rounds 3] [--out FILE]

On the synthetic database at GTDB rs214 scale (synth.config3_device) and for two sample shapes -- a 10^6-hash sample and a
real-shape 83 k-hash sample (synth.sample_device) -- five calls are timed in the same process, on the same samples:
yh_explain_device with an all-zero member table, with the overlapping references as call set 0, and totals-only
(d_flags = NULL); yh_abund_device sums-only, the yardstick (the same filter and bucket reads, an LDS hit table and
per-reference atomics where this pass has one byte read per holder and one byte written per sample hash); and
yh_run_indexed_device.  HIP events on the handle's stream around `iters` back-to-back calls that rotate through eight
samples (so the buckets come from HBM, not from a cache warmed by the previous call), after a warm-up of every call; the
calls alternate inside each of `rounds` rounds and the median round is reported with the spread.  Prints one JSON line and
writes it to --out (default profiles/residual/bench_explain.json).  Also records what writing the residual signature of a
10^6-hash sample costs on the host (residual.residual_signature + sigio.write_sig_zip).

    python scripts/bench_explain.py --batch [--batch-iters 10] [--commit ID] [--out FILE]

The batched leg alone (default --out profiles/residual/bench_explain_batch.json): blocks of 256 real-shape samples and of 32
10^6-hash samples, resident on the device as yh_run_batch_device takes them, each sample with the references it overlaps as
call set 0 of its own member row.  Two ways to the same flags and totals are timed in the same process on the same block,
alternating inside each round: (a) one yh_explain_batch_device, (b) a loop of yh_explain_device over the block's samples --
existing code, the yardstick.  Both are checked against each other before anything is timed."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yacht_amd import _lib, residual, sigio, synth  # noqa: E402
from yacht_amd.engine import RefDB  # noqa: E402

N_ROTATE = 8


def write_cost(n_hashes: int) -> dict:
    """Host seconds to cut and write the residual signature of an n-hash sample with abundances, half of it explained."""
    rng = np.random.default_rng(77)
    mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), n_hashes, dtype=np.uint64))
    sig = sigio.make_signature(mins, 31, 1000, name="s", abundances=1 + rng.integers(0, 9, mins.size))
    flags = np.where(rng.random(mins.size) < 0.5, 0x81, 0).astype(np.uint8)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        res = residual.residual_signature(sig, flags, 0, 1.0)
        t1 = time.perf_counter()
        sigio.write_sig_zip([res], os.path.join(d, residual.RESIDUAL_NAME))
        t2 = time.perf_counter()
    return {"n_hashes": int(mins.size), "n_residual": len(res.minhash), "cut_s": round(t1 - t0, 4), "write_sig_zip_s": round(t2 - t1, 4)}


def batch_leg(args) -> dict:
    """(a) yh_explain_batch_device against (b) a loop of yh_explain_device over the same resident block, us per sample."""
    import torch

    dev = torch.device("cuda:0")
    N = args.n_refs
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    result = {"bench": "explain_batch", "commit": args.commit, "n_refs": N, "n_hashes_db": int(values.numel()),
              "iters": args.batch_iters, "warmup": args.batch_warmup, "rounds": args.rounds, "tile": _lib.YH_EXPLAIN_BATCH_TILE,
              "member_rows_bytes_per_sample": N, "shapes": {}}
    for name, shape, n_sample, b in (("real_shape_83k_x256", "real", 83_000, 256), ("1e6_hash_x32", "present", 1_000_000, 32)):
        samples = [synth.sample_device(values, offsets, seed=1900 + i, n_sample=n_sample, shape=shape) for i in range(b)]
        offs = np.zeros(b + 1, dtype=np.int64)
        offs[1:] = np.cumsum([int(s.numel()) for s in samples])
        total = int(offs[-1])
        d_samples = torch.cat(samples)
        del samples
        d_offs = torch.from_numpy(offs).to(dev)
        d_abund = torch.randint(1, 1001, (total,), generator=g, device=dev, dtype=torch.int32)
        counts = torch.zeros((3, b, N), dtype=torch.int32, device=dev)
        db.run_batch_device(d_samples.data_ptr(), d_offs.data_ptr(), b, total, counts[0].data_ptr(), counts[1].data_ptr(), counts[2].data_ptr())
        db.synchronize()
        members = (counts[0] > 0).to(torch.uint8).contiguous()  # [b][N]: call set 0 of sample s = the references it overlaps
        del counts
        flags = [torch.zeros(total, dtype=torch.uint8, device=dev) for _ in range(2)]
        totals = [torch.zeros((b, 16), dtype=torch.int64, device=dev) for _ in range(2)]
        torch.cuda.synchronize()

        def batched():
            db.explain_batch_device(d_samples.data_ptr(), d_offs.data_ptr(), d_abund.data_ptr(), b, total, members.data_ptr(),
                                    flags[0].data_ptr(), totals[0].data_ptr())

        def looped():
            for s in range(b):
                o = int(offs[s])
                db.explain_device(d_samples.data_ptr() + 8 * o, d_abund.data_ptr() + 4 * o, int(offs[s + 1]) - o,
                                  members[s].data_ptr(), flags[1].data_ptr() + o, totals[1][s].data_ptr())

        batched()
        looped()
        db.synchronize()
        assert torch.equal(flags[0], flags[1]) and torch.equal(totals[0], totals[1]) and int(totals[0][:, 14].min()) > 0
        assert bool((totals[0][:, 0] == totals[0][:, 14]).all())  # every known hash is explained by the overlapping references
        calls = (("batched_us_per_sample", batched), ("looped_us_per_sample", looped))
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
        out = {"samples": b, "total_hashes": total, "hashes_in_database": int(totals[0][:, 14].sum()),
               "references_overlapping_mean": round(float(members.sum()) / b, 1), "member_rows_bytes": b * N}
        for k, v in times.items():
            out[k] = round(float(np.median(v)), 2)
            out[k.replace("_us_per_sample", "_rounds_us_per_sample")] = [round(x, 2) for x in v]
            out[k.replace("_us_per_sample", "_spread_us_per_sample")] = round(max(v) - min(v), 2)
        out["batched_over_looped"] = round(out["batched_us_per_sample"] / out["looped_us_per_sample"], 3)
        out["batched_not_slower"] = bool(out["batched_us_per_sample"] <= out["looped_us_per_sample"])
        result["shapes"][name] = out
        del d_samples, d_abund, members, flags, totals
        torch.cuda.empty_cache()
    db.close()
    return result


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="store_true", help="the batched leg alone (yh_explain_batch_device against a loop of yh_explain_device)")
    ap.add_argument("--batch-iters", type=int, default=10)
    ap.add_argument("--batch-warmup", type=int, default=3)
    ap.add_argument("--commit", default="", help="recorded in the batched leg's output")
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "residual",
                                "bench_explain_batch.json" if args.batch else "bench_explain.json")
    import torch

    assert _lib.device_count() >= 1, "bench_explain.py needs an MI355X"
    if args.batch:
        line = json.dumps(batch_leg(args))
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return
    dev = torch.device("cuda:0")
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=args.n_refs, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    N = args.n_refs
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    result = {"bench": "explain", "n_refs": N, "n_hashes_db": int(values.numel()), "iters": args.iters, "warmup": args.warmup,
              "rounds": args.rounds, "samples_rotated": N_ROTATE, "info": {k: int(v) for k, v in db.info().items()}, "shapes": {}}
    for name, shape, n_sample in (("1e6_hash", "present", 1_000_000), ("real_shape_83k", "real", 83_000)):
        samples = [synth.sample_device(values, offsets, seed=900 + i, n_sample=n_sample, shape=shape) for i in range(N_ROTATE)]
        abunds = [torch.randint(1, 1001, (int(s.numel()),), generator=g, device=dev, dtype=torch.int32) for s in samples]
        flags = torch.zeros(max(int(s.numel()) for s in samples), dtype=torch.uint8, device=dev)
        totals = torch.zeros(16, dtype=torch.int64, device=dev)
        w_ov = torch.zeros(N, dtype=torch.int64, device=dev)
        w_m = torch.zeros(N, dtype=torch.int64, device=dev)
        cnt = [torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(3)]
        member_zero = torch.zeros(N, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def run_indexed(i):
            db.run_indexed_device(samples[i].data_ptr(), int(samples[i].numel()), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())

        # call set 0 of sample i: the references that overlap it
        members = []
        for i in range(N_ROTATE):
            run_indexed(i)
            db.synchronize()
            members.append((cnt[0] > 0).to(torch.uint8))
        torch.cuda.synchronize()

        def explain_zero(i):
            db.explain_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), member_zero.data_ptr(),
                              flags.data_ptr(), totals.data_ptr())

        def explain_sets(i):
            db.explain_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), members[i].data_ptr(),
                              flags.data_ptr(), totals.data_ptr())

        def explain_totals(i):
            db.explain_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), members[i].data_ptr(), 0,
                              totals.data_ptr())

        def abund_sums(i):
            db.abundance_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), w_ov.data_ptr(), w_m.data_ptr(), 0)

        calls = (("explain_zero_member_us", explain_zero), ("explain_call_set_us", explain_sets), ("explain_totals_only_us", explain_totals),
                 ("abund_sums_only_us", abund_sums), ("run_indexed_us", run_indexed))
        # the results the timed calls produce, once, against each other: with the overlapping references as call set 0 every
        # known hash is explained, the totals-only call gives the same totals, and the known abundance is what the abundance
        # pass sums over the single-holder hits plus the shared ones
        explain_sets(0)
        db.synchronize()
        t_full, f_full = totals.clone(), flags[: int(samples[0].numel())].clone()
        explain_totals(0)
        db.synchronize()
        assert torch.equal(t_full, totals) and int(t_full[0]) == int(t_full[14]) == int((f_full >= 0x80).sum()) > 0
        assert int(t_full[1]) == int(t_full[15]) and bool(((f_full == 0) | (f_full == 0x81)).all())
        explain_zero(0)
        db.synchronize()
        assert int(totals[14]) == int(t_full[14]) and int(totals[0]) == 0
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
        shape_out = {"n_sample": int(samples[0].numel()), "references_overlapping": int(members[0].sum()),
                     "hashes_in_database": int(t_full[14])}
        for k, v in times.items():
            shape_out[k] = round(float(np.median(v)), 2)
            shape_out[k.replace("_us", "_rounds_us")] = [round(x, 2) for x in v]
        for k in ("explain_zero_member_us", "explain_call_set_us", "explain_totals_only_us"):
            shape_out[k.replace("_us", "_over_abund_sums")] = round(shape_out[k] / shape_out["abund_sums_only_us"], 3)
        spread = shape_out["abund_sums_only_rounds_us"]
        shape_out["abund_sums_spread_us"] = round(max(spread) - min(spread), 2)
        result["shapes"][name] = shape_out
    db.close()
    result["host_residual_1e6"] = write_cost(1_000_000)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
