#!/usr/bin/env python3
"""Time of the ranked set cover (yh_gather_device) and of its parts, next to the pass that makes the same reads.

    python scripts/bench_gather.py [--n-refs 85205] [--iters 50] [--warmup 5] [--rounds 3] [--out FILE]

On the synthetic database at GTDB rs214 scale (synth.config3_device) and for two sample shapes -- a real-shape 83 k-hash sample
and a 10^6-hash sample (synth.sample_device) -- with the references that overlap the sample as candidates and min_hits = 1:
  * the whole call, owners included: host clock around yh_gather_device plus the synchronize behind its owner fix-up (the
    call synchronizes the host once per chunk of rounds itself, so the host clock is what a caller waits for);
  * a pass-A call: the same call with cap_rows = 0, which runs the clear, the lookup, the count init and ONE round (a pick
    that finds the cap, a claim that finds `done`), reads the state back and synchronizes the host once -- HIP events around
    `iters` back-to-back calls, so the figure holds that host round trip; next to it yh_abund_device sums-only on the same
    samples, the same probe with another tail and no host synchronize.  Recorded, not gated.  The DEVICE time of the
    lookup kernel alone, and of the pick and claim kernels, comes from a kernel trace of this script run with
    --skip-oracle (profiles/gather/kernel_stats.txt);
  * mean time per round: (whole call - pass-A call) / rows;
  * the wall time of tests/gather_oracle.py's gather_oracle (numpy, one host core) on the same input, after its rows and
    owners were compared with the device's.
The pass-A and abundance calls rotate through four samples and alternate inside each of `rounds` rounds; the median round is
reported with the spread.  Prints one JSON line and writes it to --out (default profiles/gather/bench_gather.json).

    python scripts/bench_gather.py --batch [--n-refs 85205] [--rounds 3] [--batch-caps 64 1024] [--skip-loop] [--out FILE]

--batch times ONE yh_gather_batch_device over a resident block against a LOOP of the unchanged yh_gather_device over the same
block: the same samples, abundances and candidates (the references that overlap each sample, as bit 0 of the member rows),
min_hits 1, no owners.  Blocks: 256 real-shape 83 k-hash samples, and 32 samples of 10^6 hashes; cap_rows 64 and 1024.
Both are timed with the host clock from the first call to the end of a synchronize -- the looped call synchronizes the host
itself, so that is what a caller of either waits for -- and reported in us per sample: the median of `rounds` rounds with the
spread.  Before anything is timed every sample's count, `more` and rows must equal the looped call's.  --skip-loop runs the
batched calls alone (for a kernel trace: profiles/gather/kernel_stats_batch.txt).  Default --out:
profiles/gather/bench_gather_batch.json."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gather_oracle import gather_oracle  # noqa: E402

from yacht_amd import _lib, engine, synth  # noqa: E402
from yacht_amd.engine import RefDB  # noqa: E402

N_ROTATE = 4


def batch_main(args) -> None:
    import torch

    assert _lib.device_count() >= 1, "bench_gather.py needs an MI355X"
    dev = torch.device("cuda:0")
    N = args.n_refs
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    result = {"bench": "gather_batch", "n_refs": N, "n_hashes_db": int(values.numel()), "rounds": args.rounds, "min_hits": 1,
              "owners": False, "clock": "host, first call to the end of a synchronize", "loop_skipped": bool(args.skip_loop), "blocks": {}}
    ok = True
    for name, shape, n_sample, b in (("256_real_shape_83k", "real", 83_000, 256), ("32_of_1e6_hashes", "present", 1_000_000, 32)):
        b = min(b, args.batch_samples) if args.batch_samples else b
        samples = [synth.sample_device(values, offsets, seed=900 + i, n_sample=n_sample, shape=shape) for i in range(b)]
        sizes = [int(s.numel()) for s in samples]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total = int(offs[-1])
        d_s = torch.cat(samples)
        d_o = torch.from_numpy(offs).to(dev)
        d_a = torch.randint(1, 1001, (total,), generator=g, device=dev, dtype=torch.int32)
        members = torch.zeros((b, N), dtype=torch.uint8, device=dev)
        cnt = [torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(3)]
        for i in range(b):  # the candidates of sample i: the references that overlap it
            db.run_indexed_device(samples[i].data_ptr(), sizes[i], cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())
            db.synchronize()
            members[i] = (cnt[0] > 0).to(torch.uint8)
        torch.cuda.synchronize()
        block = {"samples": b, "total_hashes": total, "candidates_mean": round(float(members.sum()) / b, 1), "caps": {}}
        for cap in args.batch_caps:
            rows_b = torch.zeros((b, cap, 3), dtype=torch.int64, device=dev)
            rows_l = torch.zeros((b, cap, 3), dtype=torch.int64, device=dev)
            n_b = torch.zeros(b, dtype=torch.int32, device=dev)
            more_b = torch.zeros(b, dtype=torch.uint8, device=dev)

            def batched():
                t0 = time.perf_counter()
                db.gather_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), b, total, members.data_ptr(), 1, 1, rows_b.data_ptr(),
                                       cap, 0, n_b.data_ptr(), more_b.data_ptr())
                db.synchronize()
                return (time.perf_counter() - t0) * 1e6 / b

            def looped():
                got = []
                t0 = time.perf_counter()
                for i in range(b):
                    got.append(db.gather_device(d_s.data_ptr() + 8 * int(offs[i]), d_a.data_ptr() + 4 * int(offs[i]), sizes[i],
                                                members[i].data_ptr(), 1, rows_l[i].data_ptr(), cap, 0))
                db.synchronize()
                return (time.perf_counter() - t0) * 1e6 / b, got

            out = {}
            with torch.cuda.stream(stream):
                batched()  # (warm: the working memory comes from the buffer cache afterwards)
                if not args.skip_loop:
                    _, got = looped()
                    torch.cuda.synchronize()
                    n_rows, more = n_b.cpu().numpy(), more_b.cpu().numpy()
                    assert [int(x) for x in n_rows] == [k for k, _ in got] and [bool(x) for x in more] == [m for _, m in got], (name, cap)
                    hb, hl = rows_b.cpu().numpy(), rows_l.cpu().numpy()
                    assert all(np.array_equal(hb[i, :k], hl[i, :k]) for i, (k, _) in enumerate(got)), (name, cap)
                    out["rows_equal_the_looped_calls"] = True
                    out["rows_mean"] = round(float(n_rows.mean()), 1)
                    out["samples_cut_at_the_cap"] = int(more.sum())
                tb = [batched() for _ in range(args.rounds)]
                tl = [looped()[0] for _ in range(args.rounds)] if not args.skip_loop else []
            out["batched_us_per_sample"] = round(float(np.median(tb)), 2)
            out["batched_rounds_us_per_sample"] = [round(x, 2) for x in tb]
            out["rounds_enqueued"] = min(cap, N) + 1
            if tl:
                out["looped_us_per_sample"] = round(float(np.median(tl)), 2)
                out["looped_rounds_us_per_sample"] = [round(x, 2) for x in tl]
                out["looped_over_batched"] = round(out["looped_us_per_sample"] / out["batched_us_per_sample"], 2)
                out["batched_no_slower"] = out["batched_us_per_sample"] <= out["looped_us_per_sample"]
                ok = ok and out["batched_no_slower"]
            else:
                out["looped_us_per_sample"] = None  # unmeasured: --skip-loop
            block["caps"][str(cap)] = out
            del rows_b, rows_l
        result["blocks"][name] = block
        del samples, d_s, d_a, members
    result["accepted"] = None if args.skip_loop else ok
    db.close()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not args.skip_loop and not ok:
        sys.exit("batched us per sample above looped us per sample")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-oracle", action="store_true", help="no host oracle and no comparison with it (for a profiler run)")
    ap.add_argument("--batch", action="store_true", help="yh_gather_batch_device against a loop of yh_gather_device")
    ap.add_argument("--batch-caps", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--batch-samples", type=int, default=0, help="at most this many samples per block (0: 256 and 32)")
    ap.add_argument("--skip-loop", action="store_true", help="--batch: the batched calls alone (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gather", "bench_gather_batch.json" if args.batch else "bench_gather.json")
    if args.batch:
        return batch_main(args)
    import torch

    assert _lib.device_count() >= 1, "bench_gather.py needs an MI355X"
    dev = torch.device("cuda:0")
    N = args.n_refs
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    h_values = values.cpu().numpy().view(np.uint64)
    h_offsets = offsets.cpu().numpy().view(np.uint64)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    result = {"bench": "gather", "n_refs": N, "n_hashes_db": int(values.numel()), "iters": args.iters, "warmup": args.warmup,
              "rounds": args.rounds, "samples_rotated": N_ROTATE, "rounds_per_sync": _lib.YH_GATHER_ROUNDS_PER_SYNC,
              "host_cores_used_by_oracle": 1, "host_cores_available": len(os.sched_getaffinity(0)), "shapes": {}}
    for name, shape, n_sample in (("real_shape_83k", "real", 83_000), ("1e6_hash", "present", 1_000_000)):
        samples = [synth.sample_device(values, offsets, seed=900 + i, n_sample=n_sample, shape=shape) for i in range(N_ROTATE)]
        abunds = [torch.randint(1, 1001, (int(s.numel()),), generator=g, device=dev, dtype=torch.int32) for s in samples]
        cnt = [torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(3)]
        w_ov = torch.zeros(N, dtype=torch.int64, device=dev)
        w_m = torch.zeros(N, dtype=torch.int64, device=dev)
        rows = torch.zeros((N, 3), dtype=torch.int64, device=dev)
        owner = torch.zeros(max(int(s.numel()) for s in samples), dtype=torch.int32, device=dev)
        cands = []
        for i in range(N_ROTATE):  # the candidates of sample i: the references that overlap it
            db.run_indexed_device(samples[i].data_ptr(), int(samples[i].numel()), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())
            db.synchronize()
            cands.append((cnt[0] > 0).to(torch.uint8))
        torch.cuda.synchronize()

        def gather_full(i):
            got = db.gather_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), cands[i].data_ptr(), 1,
                                   rows.data_ptr(), N, owner.data_ptr())
            db.synchronize()
            return got

        def pass_a(i):
            db.gather_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), cands[i].data_ptr(), 1, rows.data_ptr(), 0, 0)

        def abund_sums(i):
            db.abundance_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), w_ov.data_ptr(), w_m.data_ptr(), 0)

        # the device's answer for sample 0 against the host oracle, which is timed on the way
        n_rows, more = gather_full(0)
        got_rows = rows.cpu().numpy().view(engine.GATHER_ROW_DTYPE).reshape(-1)[:n_rows].copy()
        got_owner = owner[: int(samples[0].numel())].cpu().numpy().view(np.uint32)
        h_sample = samples[0].cpu().numpy().view(np.uint64)
        h_abund, h_cand = abunds[0].cpu().numpy().view(np.uint32), cands[0].cpu().numpy()
        stats = {"n_shared_live": None, "n_solo_candidate": None, "n_tie_rounds": None}
        oracle_s = None
        if not args.skip_oracle:
            t0 = time.perf_counter()
            want = gather_oracle(h_values, h_offsets, h_sample, h_cand, h_abund, stats=stats)
            oracle_s = time.perf_counter() - t0
            assert not more and np.array_equal(got_rows, want[0]) and np.array_equal(got_owner, want[2]), name
        with torch.cuda.stream(stream):
            for i in range(args.warmup):
                pass_a(i % N_ROTATE)
                abund_sums(i % N_ROTATE)
            gather_full(0)
            whole = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                gather_full(0)
                whole.append((time.perf_counter() - t0) * 1e6)
            times = {"pass_a_call_us": [], "abund_sums_only_us": []}
            for _ in range(args.rounds):
                for k, fn in (("pass_a_call_us", pass_a), ("abund_sums_only_us", abund_sums)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for i in range(args.iters):
                        fn(i % N_ROTATE)
                    e1.record(stream)
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        out = {"n_sample": int(samples[0].numel()), "candidates": int(h_cand.sum()), "rows": int(n_rows),
               "live_list_length": stats["n_shared_live"], "single_holder_hits_on_candidates": stats["n_solo_candidate"],
               "rounds_decided_by_the_tie_rule": stats["n_tie_rounds"], "host_syncs": -(-(int(n_rows) + 1) // _lib.YH_GATHER_ROUNDS_PER_SYNC),
               "whole_call_us": round(float(np.median(whole)), 1), "whole_call_rounds_us": [round(x, 1) for x in whole],
               "host_oracle_s": None if oracle_s is None else round(oracle_s, 3)}
        for k, v in times.items():
            out[k] = round(float(np.median(v)), 2)
            out[k.replace("_us", "_rounds_us")] = [round(x, 2) for x in v]
        out["pass_a_call_over_abund_sums"] = round(out["pass_a_call_us"] / out["abund_sums_only_us"], 3)
        out["mean_round_us"] = round((out["whole_call_us"] - out["pass_a_call_us"]) / max(int(n_rows), 1), 2)
        if oracle_s is not None:
            out["host_oracle_over_whole_call"] = round(oracle_s * 1e6 / out["whole_call_us"], 1)
        result["shapes"][name] = out
    db.close()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
