#!/usr/bin/env python3
"""The segmented sketch (yh_sketch_segments*) next to what it replaces.  Three legs, each writes one JSON file under
profiles/sketch_segments/ (--out-dir) and prints it as one line:

    python scripts/bench_sketch_segments.py kernel   [--mbases 256] [--iters 10] [--rounds 3]
    python scripts/bench_sketch_segments.py call     [--records 2000] [--record-kb 50] [--rounds 3]
    python scripts/bench_sketch_segments.py command  [--records 2000] [--record-kb 50] [--genomes 256] [--genome-mb 2]

kernel   A resident buffer of random bases, k = 31 and 51, scaled 1000.  HIP events around `iters` back-to-back calls, the
         calls alternating inside each round, the median round with the spread: yh_sketch_dna_device (the unsegmented
         kernel), yh_sketch_segments_device with one segment and with segments of about 5 kb -- whole (hashing, two sorts,
         flags, scan, emit, offsets) and with cap_kept = 0, which runs the hashing kernel with its segment lookups but
         stores no pair and sorts nothing: `hash_ms`.  `tail_ms` = whole - hash, the sorts and the run-length launches.
         Before anything is timed the segmented result must equal torch's own sort / unique of the unsegmented hashes.
call     One MAG-like buffer of `records` records: one yh_sketch_segments against the loop of yh_sketch_dna + np.unique per
         record that `yacht sketch ref` made before, at scaled 1000 and 10, host clock, results compared first.
command  `yacht sketch ref` in a child process on that file and on a folder of synthetic gzip genomes: default path against
         YACHT_SKETCH_REF=loop, wall time, ONE run each (no spread).  The phases are timed in this process on the same
         inputs: read + decompress (one thread, and the reader pool), device (sketch_units on units already in memory), write."""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yacht_amd import _lib, sigio, sketch  # noqa: E402


def _median_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


# ---- kernel ------------------------------------------------------------------------------------------------------------------
def leg_kernel(args) -> dict:
    import torch

    lib = _lib.load()
    n = args.mbases * 1_000_000
    gen = torch.Generator(device="cuda").manual_seed(5)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    seq = acgt[torch.randint(0, 4, (n,), generator=gen, device="cuda")]
    assert seq.data_ptr() % 16 == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mh = sketch.max_hash_for_scaled(1000)
    cap = int(n / 1000 * 1.25) + 4096
    n_many = max(n // 5000, 1)
    rng = np.random.default_rng(6)
    cuts = np.sort(rng.integers(0, n, size=n_many - 1)).astype(np.uint64)
    tables = {"one": np.array([0, n], dtype=np.uint64), "many": np.concatenate(([0], cuts, [n])).astype(np.uint64)}
    d_tables = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in tables.items()}
    wb = int(lib.yh_sketch_segments_work_bytes(cap, n_many))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    hashes = torch.empty(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    mins = torch.empty(cap, dtype=torch.int64, device="cuda")
    abund = torch.empty(cap, dtype=torch.int32, device="cuda")
    off = torch.empty(n_many + 1, dtype=torch.int64, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")

    def unseg(k):
        _lib.check(lib.yh_sketch_dna_device(C.c_void_p(seq.data_ptr()), n, k, 42, mh, cap, C.c_void_p(hashes.data_ptr()),
                                            C.c_void_p(count.data_ptr()), stream))

    def seg(k, which, cap_kept):
        t = d_tables[which]
        _lib.check(lib.yh_sketch_segments_device(C.c_void_p(seq.data_ptr()), n, C.c_void_p(t.data_ptr()), t.numel() - 1, k, 42, mh, cap_kept,
                                                 C.c_void_p(work.data_ptr()), wb, cap if cap_kept else 0, C.c_void_p(mins.data_ptr()),
                                                 C.c_void_p(abund.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(totals.data_ptr()), stream))

    out = {"leg": "kernel", "bases": n, "scaled": 1000, "segments_many": n_many, "iters": args.iters, "rounds": args.rounds, "clock": "HIP events",
           "device": torch.cuda.get_device_name(0), "k": {}}
    for k in (31, 51):
        # correctness first: one segment = the unsegmented hashes sorted and counted; many segments lose only boundary windows
        unseg(k)
        seg(k, "one", cap)
        torch.cuda.synchronize()
        c = int(count.item())
        assert c <= cap
        u, cnt = torch.unique(hashes[:c], return_counts=True)     # (int64 view: order differs from uint64 only past 2^63 > max_hash)
        t = [int(x) for x in totals.cpu()]
        assert t == [c, u.numel()] and torch.equal(mins[:t[1]], u) and torch.equal(abund[:t[1]].long(), cnt), "segmented result differs"
        seg(k, "many", cap)
        torch.cuda.synchronize()
        t_many = [int(x) for x in totals.cpu()]
        assert 0.95 * c < t_many[0] <= c and int(off[-1].item()) == t_many[1]
        calls = {"unsegmented": lambda: unseg(k), "seg_one": lambda: seg(k, "one", cap), "seg_one_hash": lambda: seg(k, "one", 0),
                 "seg_many": lambda: seg(k, "many", cap), "seg_many_hash": lambda: seg(k, "many", 0)}
        for f in calls.values():
            f()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(args.rounds):
            for name, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _i in range(args.iters):
                    f()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / args.iters)
        r = {name + "_ms": _median_spread(v) for name, v in ms.items()}
        base = r["unsegmented_ms"]["median"]
        spread = max((v["max"] - v["min"]) / v["median"] for v in r.values())
        for which in ("one", "many"):
            r[f"seg_{which}_tail_ms"] = round(r[f"seg_{which}_ms"]["median"] - r[f"seg_{which}_hash_ms"]["median"], 4)
            r[f"seg_{which}_hash_over_unsegmented"] = round(r[f"seg_{which}_hash_ms"]["median"] / base, 4)
        r["kept"] = c
        r["kept_many"] = t_many[0]
        r["largest_relative_spread"] = round(spread, 4)
        r["gbases_per_s_unsegmented"] = round(n / base / 1e6, 1)
        out["k"][str(k)] = r
    return out


# ---- call --------------------------------------------------------------------------------------------------------------------
def _records(n_records, record_kb, seed=7):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [acgt[rng.integers(0, 4, size=record_kb * 1000)].tobytes() for _ in range(n_records)]


def leg_call(args) -> dict:
    recs = _records(args.records, args.record_kb)
    buf = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = np.arange(args.records + 1, dtype=np.uint64) * np.uint64(args.record_kb * 1000)
    out = {"leg": "call", "records": args.records, "record_bases": args.record_kb * 1000, "k": 31, "rounds": args.rounds, "clock": "host", "scaled": {}}
    for scaled in (1000, 10):
        def batched():
            return sketch.sketch_segments(buf, off, 31, scaled)

        def loop():
            return [sketch.sketch_sequences([r], 31, scaled) for r in recs]

        m, a, o = batched()
        ref = loop()
        assert int(o[-1]) == sum(x[0].size for x in ref)
        for s, (rm, ra) in enumerate(ref):
            assert np.array_equal(m[int(o[s]):int(o[s + 1])], rm) and np.array_equal(a[int(o[s]):int(o[s + 1])], ra.astype(np.uint32))
        t = {"batched_s": [], "loop_s": []}
        for _ in range(args.rounds):
            for name, f in (("batched_s", batched), ("loop_s", loop)):
                t0 = time.perf_counter()
                f()
                t[name].append(time.perf_counter() - t0)
        r = {name: _median_spread(v) for name, v in t.items()}
        r["loop_over_batched"] = round(r["loop_s"]["median"] / r["batched_s"]["median"], 2)
        r["mins"] = int(o[-1])
        out["scaled"][str(scaled)] = r
    return out


# ---- command -----------------------------------------------------------------------------------------------------------------
def _write_genome(job):
    path, seed, n = job
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with gzip.open(path, "wb", compresslevel=1) as f:
        for c in range(4):
            f.write(b">contig%d\n" % c)
            f.write(acgt[rng.integers(0, 4, size=n // 4)].tobytes() + b"\n")


def _run_cli(infile, outfile, scaled, loop):
    env = dict(os.environ)
    env.pop("YACHT_SKETCH_REF", None)
    if loop:
        env["YACHT_SKETCH_REF"] = "loop"
    t0 = time.perf_counter()
    subprocess.run([sys.executable, "-m", "yacht_amd.cli", "sketch", "ref", "--infile", infile, "--kmer", "31", "--scaled", str(scaled),
                    "--outfile", outfile], check=True, env=env, cwd=ROOT)
    return round(time.perf_counter() - t0, 3)


def leg_command(args) -> dict:
    out = {"leg": "command", "clock": "wall, one run each: no spread", "k": 31}
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "mag.fa")
        recs = _records(args.records, args.record_kb)
        with open(fa, "wb") as f:
            for i, r in enumerate(recs):
                f.write(b">scaffold%d\n" % i + r + b"\n")
        gdir = os.path.join(tmp, "genomes")
        os.makedirs(gdir)
        jobs = [(os.path.join(gdir, f"g{i:04d}.fna.gz"), 1000 + i, args.genome_mb * 1_000_000) for i in range(args.genomes)]
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(_write_genome, jobs))
        for scaled in (1000, 10):
            a = _run_cli(fa, os.path.join(tmp, "a.zip"), scaled, False)
            b = _run_cli(fa, os.path.join(tmp, "b.zip"), scaled, True)
            sa, sb = sigio.load_file_as_signatures(os.path.join(tmp, "a.zip"), ksize=31), sigio.load_file_as_signatures(os.path.join(tmp, "b.zip"), ksize=31)
            assert [s.md5sum() for s in sa] == [s.md5sum() for s in sb] and [s.name for s in sa] == [s.name for s in sb]
            out[f"file_scaled{scaled}"] = {"records": args.records, "record_bases": args.record_kb * 1000, "default_s": a, "loop_s": b,
                                           "loop_over_default": round(b / a, 2)}
        a = _run_cli(gdir, os.path.join(tmp, "a.zip"), 1000, False)
        b = _run_cli(gdir, os.path.join(tmp, "b.zip"), 1000, True)
        sa, sb = sigio.load_file_as_signatures(os.path.join(tmp, "a.zip"), ksize=31), sigio.load_file_as_signatures(os.path.join(tmp, "b.zip"), ksize=31)
        assert [s.md5sum() for s in sa] == [s.md5sum() for s in sb] and [s.name for s in sa] == [s.name for s in sb]
        folder = {"genomes": args.genomes, "genome_bases": args.genome_mb * 1_000_000, "scaled": 1000, "default_s": a, "loop_s": b,
                  "loop_over_default": round(b / a, 2)}
        # the phases, in this process
        paths = [j[0] for j in jobs]
        t0 = time.perf_counter()
        units = [sketch._read_unit(p)[1] for p in paths]
        folder["read_one_thread_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        n_read = sum(1 for _ in sketch.read_units_ahead(paths, sketch.batch_bytes()))
        folder["read_pool_s"] = round(time.perf_counter() - t0, 3)
        assert n_read == len(paths)
        list(sketch.sketch_units(units[:2], 31, 1000))  # (warm: buffers, code objects)
        t0 = time.perf_counter()
        sk = list(sketch.sketch_units(units, 31, 1000))
        folder["device_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        sigs = [sigio.Signature(sigio.MinHash(m, 31, sketch.max_hash_for_scaled(1000), ab), name=str(i)) for i, (m, ab) in enumerate(sk)]
        sigio.write_sig_zip(sigs, os.path.join(tmp, "c.zip"))
        folder["write_s"] = round(time.perf_counter() - t0, 3)
        folder["bound_by"] = "read + decompress on the host" if folder["read_pool_s"] > folder["device_s"] else "device"
        out["folder"] = folder
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("leg", choices=("kernel", "call", "command"))
    ap.add_argument("--mbases", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--record-kb", type=int, default=50)
    ap.add_argument("--genomes", type=int, default=256)
    ap.add_argument("--genome-mb", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "sketch_segments"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_sketch_segments.py needs a HIP device: nothing is measured without one")
    res = {"kernel": leg_kernel, "call": leg_call, "command": leg_command}[args.leg](args)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, f"bench_{args.leg}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
