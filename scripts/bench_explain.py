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
10^6-hash sample costs on the host (residual.residual_signature + sigio.write_sig_zip)."""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "residual",
                                                  "bench_explain.json"))
    args = ap.parse_args()
    import torch

    assert _lib.device_count() >= 1, "bench_explain.py needs an MI355X"
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
