#!/usr/bin/env python3
"""`yacht sketch sample` streamed through the device accumulator (yh_sketch_acc*) next to the path it replaces
(YACHT_SKETCH_SAMPLE=whole).  Every leg merges its result into ONE file, <out-dir>/bench_sketch_sample.json (default
profiles/sketch_sample/); a leg that has not been run stays in it as "unmeasured".

    python scripts/bench_sketch_sample.py device   [--mbases 1000] [--rounds 3] [--only acc]
    python scripts/bench_sketch_sample.py command  [--mb 2000] [--rounds 3] [--streamed-only]
    python scripts/bench_sketch_sample.py trace    --stats-csv <kernel_stats.csv of a `device --only acc` run under a kernel trace>

device   `mbases` of synthetic 150-base reads, one per line, resident in HBM, scaled 1000, k = 31.  The accumulator takes them
         in chunks of 256 MiB (cut at read boundaries, 16-byte aligned) through yh_sketch_acc_add_device and is finished; the
         comparison is the device work of the unchanged path on the same bytes: one yh_sketch_dna_device over everything and
         torch's sort / unique of the kept hashes.  The two must give the same hashes and counts before anything is timed.
         HIP events around each, the two alternating, median of `rounds` with the spread.  (Every accumulator call returns
         with its work done, so its figure includes one host round trip per chunk.)
command  A synthetic gzip FASTQ of `mb` MB uncompressed and one of a quarter of that; `yacht sketch sample` in a child
         process, default against whole, alternating, `rounds` each: wall time, peak RSS of the child (getrusage), and the
         read / device / write phases.  The child makes main_sample's calls itself, with a clock between them (streamed:
         `read` is the time spent waiting for the reader thread).  The two outputs must be the same archive byte for byte.
trace    The compaction's share of the accumulator's kernel time, from the per-kernel totals of a kernel trace."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import resource
import statistics
import subprocess
import sys
import tempfile
import time
import zipfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yacht_amd import _lib, sigio, sketch  # noqa: E402

READ_LEN = 150
CHUNK_BYTES = 256 << 20


def _median_spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _rel_spread(d):
    return (d["max"] - d["min"]) / d["median"] if d["median"] else 0.0


def _verdict(new, old, what):
    """`new` no larger than `old`, judged with 10 % or the rounds' spread, whichever is larger"""
    margin = max(0.10, _rel_spread(new), _rel_spread(old))
    ratio = new["median"] / old["median"]
    return {"what": what, "ratio": round(ratio, 4), "margin": round(margin, 4), "verdict": "shown" if ratio <= 1.0 + margin else "refuted"}


# ---- device ------------------------------------------------------------------------------------------------------------------
def leg_device(args) -> dict:
    import torch

    lib = _lib.load()
    stride = READ_LEN + 1
    n_reads = args.mbases * 1_000_000 // READ_LEN
    n = n_reads * stride
    gen = torch.Generator(device="cuda").manual_seed(5)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    seq = acgt[torch.randint(0, 4, (n,), generator=gen, device="cuda", dtype=torch.uint8).long()]
    seq[READ_LEN::stride] = ord("\n")
    assert seq.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    per_chunk = CHUNK_BYTES // (16 * stride) * (16 * stride)   # whole reads, and every chunk starts 16-byte aligned
    cuts = list(range(0, n, per_chunk)) + [n]
    mh = sketch.max_hash_for_scaled(1000)
    cap = int(n / 1000 * 1.25) + 4096
    hashes = torch.empty(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def whole():
        _lib.check(lib.yh_sketch_dna_device(C.c_void_p(seq.data_ptr()), n, 31, 42, mh, cap, C.c_void_p(hashes.data_ptr()),
                                            C.c_void_p(count.data_ptr()), stream))
        c = int(count.item())
        assert c <= cap
        return torch.unique(hashes[:c], return_counts=True)   # (int64 view: the order differs from uint64 only past 2^63 > max_hash)

    def acc_run(acc):
        for a, b in zip(cuts[:-1], cuts[1:]):
            acc.add_device(seq.data_ptr() + a, b - a - 1)     # (without the last newline)
        return acc.finish_device()

    # the same result first (a traced run, --only acc, keeps torch's own sort kernels out of the trace: no comparison there)
    with sketch.SketchAccumulator(31, 1000) as acc:
        acc_run(acc)
        mins, counts = acc.finish()
        info = acc.info()
    if args.only != "acc":
        u, cnt = whole()
        assert np.array_equal(mins.view(np.int64), u.cpu().numpy()) and np.array_equal(counts.view(np.int64), cnt.cpu().numpy()), "results differ"
    out = {"leg": "device", "bases": n_reads * READ_LEN, "bytes": n, "reads": n_reads, "chunks": len(cuts) - 1, "chunk_bytes": per_chunk,
           "scaled": 1000, "k": 31, "kept": info["n_kept"], "distinct": int(mins.size), "compactions": info["n_compactions"],
           "rehashed_chunks": info["n_rehashed_chunks"], "rounds": args.rounds, "clock": "HIP events", "device": torch.cuda.get_device_name(0)}
    ms = {"accumulator_ms": [], "whole_ms": []}
    for _ in range(args.rounds):
        for name in ms:
            if name == "whole_ms" and args.only == "acc":
                continue
            acc = sketch.SketchAccumulator(31, 1000) if name == "accumulator_ms" else None
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if acc is not None:
                acc_run(acc)
            else:
                whole()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
            if acc is not None:
                acc.close()
    out["accumulator_ms"] = _median_spread(ms["accumulator_ms"])
    if ms["whole_ms"]:
        out["whole_ms"] = _median_spread(ms["whole_ms"])
        out["expectation_accumulator_no_slower"] = _verdict(out["accumulator_ms"], out["whole_ms"], "accumulator_ms / whole_ms")
    return out


# ---- trace -------------------------------------------------------------------------------------------------------------------
def leg_trace(args) -> dict:
    hashing = compaction = other = 0.0
    names = {}
    with open(args.stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            names[name[:80]] = names.get(name[:80], 0.0) + ns
            if "k_sketch_dna" in name:
                hashing += ns
            elif "k_acc_" in name or "rocprim" in name:
                compaction += ns
            else:
                other += ns
    total = hashing + compaction   # (other: the kernels that made the synthetic reads)
    return {"leg": "trace", "source": "kernel trace of `device --only acc`, per-kernel totals", "hashing_ms": round(hashing / 1e6, 4),
            "compaction_ms": round(compaction / 1e6, 4), "other_ms": round(other / 1e6, 4),
            "compaction_share_of_accumulator_kernel_time": round(compaction / total, 4) if total else None,
            "kernels_ms": {k: round(v / 1e6, 4) for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:12]}}


# ---- command -----------------------------------------------------------------------------------------------------------------
def _write_fastq_gz(path, n_reads, seed):
    """n_reads 150-base reads as gzip FASTQ: independent gzip members of 64k reads, compressed by a thread pool"""
    header = 12   # "@r" + nine digits + "\n"
    rec = header + READ_LEN + 1 + 2 + READ_LEN + 1
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def member(job):
        first, count = job
        rng = np.random.default_rng((seed, first))
        a = np.empty((count, rec), dtype=np.uint8)
        a[:, 0] = ord("@")
        a[:, 1] = ord("r")
        ids = np.arange(first, first + count)
        for d in range(9):
            a[:, 10 - d] = ord("0") + (ids // 10 ** d) % 10
        a[:, 11] = ord("\n")
        a[:, header:header + READ_LEN] = acgt[rng.integers(0, 4, size=(count, READ_LEN))]
        o = header + READ_LEN
        a[:, o] = ord("\n")
        a[:, o + 1] = ord("+")
        a[:, o + 2] = ord("\n")
        a[:, o + 3:o + 3 + READ_LEN] = ord("I")
        a[:, rec - 1] = ord("\n")
        if count > 100:   # some reads twice: abundances above 1
            a[1:count:50, header:header + READ_LEN] = a[0:count - 1:50, header:header + READ_LEN]
        z = zlib.compressobj(1, zlib.DEFLATED, 31)
        return z.compress(a.tobytes()) + z.flush()

    jobs = [(i, min(65536, n_reads - i)) for i in range(0, n_reads, 65536)]
    with ThreadPoolExecutor(max_workers=16) as pool, open(path, "wb") as f:
        for blob in pool.map(member, jobs):
            f.write(blob)
    return n_reads * rec


CHILD = r"""
import json, os, resource, sys, time
sys.path.insert(0, sys.argv[1])
t_start = time.perf_counter()
import numpy as np
from yacht_amd import sigio, sketch
infile, outfile = sys.argv[2], sys.argv[3]
ph = {"read_s": 0.0, "device_s": 0.0, "write_s": 0.0}
mh = sketch.max_hash_for_scaled(1000)
if sketch.use_whole_sample_path():
    t0 = time.perf_counter()
    seqs = [s for _n, s in sketch.read_sequences(infile)]
    t1 = time.perf_counter()
    mins, ab = sketch.sketch_sequences(seqs, 31, 1000)
    t2 = time.perf_counter()
    ph["read_s"], ph["device_s"] = t1 - t0, t2 - t1   # (device: the join, the call and np.unique)
else:
    with sketch.SketchAccumulator(31, 1000) as acc:
        it = sketch.read_chunks_ahead([infile], sketch.batch_bytes())
        while True:
            t0 = time.perf_counter()
            chunk = next(it, None)
            t1 = time.perf_counter()
            ph["read_s"] += t1 - t0                     # (waiting for the reader thread)
            if chunk is None:
                break
            acc.add(chunk)
            ph["device_s"] += time.perf_counter() - t1
        t1 = time.perf_counter()
        mins, counts = acc.finish()
        ab = counts.astype(np.int64)
        ph["device_s"] += time.perf_counter() - t1
t0 = time.perf_counter()
sig = sigio.Signature(sigio.MinHash(mins, 31, mh, ab), name=os.path.basename(infile), filename=infile)
sigio.write_sig_zip([sig], outfile)
ph["write_s"] = time.perf_counter() - t0
ph["total_s"] = time.perf_counter() - t_start
print("PHASES " + json.dumps({k: round(v, 3) for k, v in ph.items()}), flush=True)
"""


def _same_archive(a, b):
    with zipfile.ZipFile(a) as za, zipfile.ZipFile(b) as zb:
        return za.namelist() == zb.namelist() and all(za.read(n) == zb.read(n) for n in za.namelist())


def _child_rss(infile, outfile, whole):
    """peak RSS of ONE child, exactly: the child is started through a wrapper process whose own children are only it"""
    code = ("import resource, subprocess, sys; subprocess.run(sys.argv[1:], check=True); "
            "print('RSS', resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss)")
    env = dict(os.environ)
    env.pop("YACHT_SKETCH_SAMPLE", None)
    env.pop("YACHT_SKETCH_BATCH_BYTES", None)
    if whole:
        env["YACHT_SKETCH_SAMPLE"] = "whole"
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-c", code, sys.executable, "-c", CHILD, ROOT, infile, outfile], check=True, env=env, cwd=ROOT,
                       capture_output=True, text=True)
    wall = time.perf_counter() - t0
    rss_kb = int([ln for ln in p.stdout.splitlines() if ln.startswith("RSS ")][-1].split()[1])
    phases = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("PHASES ")][-1][7:])
    return wall, rss_kb / 1024.0, phases


def leg_command(args) -> dict:
    out = {"leg": "command", "k": 31, "scaled": 1000, "rounds": args.rounds, "clock": "wall of a child process; peak RSS: getrusage of that child",
           "files": {}}
    rec = 12 + READ_LEN + 1 + 2 + READ_LEN + 1
    with tempfile.TemporaryDirectory(dir=args.tmp_dir) as tmp:
        for label, mb in (("small", args.mb // 4), ("large", args.mb)):
            path = os.path.join(tmp, f"{label}.fq.gz")
            n_reads = mb * 1_000_000 // rec
            t0 = time.perf_counter()
            raw = _write_fastq_gz(path, n_reads, seed=11)
            r = {"reads": n_reads, "uncompressed_bytes": raw, "gzip_bytes": os.path.getsize(path), "made_in_s": round(time.perf_counter() - t0, 1)}
            modes = ("streamed",) if args.streamed_only else ("streamed", "whole")
            runs = {mode: {"wall_s": [], "rss_mb": [], "phases": []} for mode in modes}
            for i in range(args.rounds):
                for mode in modes:
                    o = os.path.join(tmp, f"{label}_{mode}.sig.zip")
                    wall, rss, phases = _child_rss(path, o, mode == "whole")
                    runs[mode]["wall_s"].append(wall)
                    runs[mode]["rss_mb"].append(rss)
                    runs[mode]["phases"].append(phases)
                    print(f"{label} round {i} {mode}: {wall:.1f} s, {rss:.0f} MB", file=sys.stderr, flush=True)
                if i == 0 and not args.streamed_only:
                    assert _same_archive(os.path.join(tmp, f"{label}_streamed.sig.zip"), os.path.join(tmp, f"{label}_whole.sig.zip")), "archives differ"
                    sig = sigio.load_file_as_signatures(os.path.join(tmp, f"{label}_whole.sig.zip"), ksize=31)[0]
                    r["mins"], r["max_abundance"] = len(sig.minhash), int(sig.minhash.abundances.max())
            for mode, v in runs.items():
                r[mode] = {"wall_s": _median_spread(v["wall_s"]), "peak_rss_mb": _median_spread(v["rss_mb"]),
                           "phases_s": {k: _median_spread([p[k] for p in v["phases"]]) for k in v["phases"][0]}}
            if not args.streamed_only:
                r["expectation_streamed_wall_no_longer"] = _verdict(r["streamed"]["wall_s"], r["whole"]["wall_s"], "streamed wall / whole wall")
            out["files"][label] = r
        s, l = out["files"]["small"], out["files"]["large"]
        grow = l["streamed"]["peak_rss_mb"]["median"] / s["streamed"]["peak_rss_mb"]["median"]
        margin = max(_rel_spread(l["streamed"]["peak_rss_mb"]), _rel_spread(s["streamed"]["peak_rss_mb"]))
        out["expectation_streamed_rss_does_not_grow"] = {"what": "streamed peak RSS, large / small (the input grows fourfold)", "ratio": round(grow, 4),
                                                         "margin": round(margin, 4), "verdict": "shown" if grow <= 1.0 + margin else "refuted"}
        if not args.streamed_only:
            out["whole_rss_large_over_small"] = round(l["whole"]["peak_rss_mb"]["median"] / s["whole"]["peak_rss_mb"]["median"], 3)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("leg", choices=("device", "command", "trace"))
    ap.add_argument("--mbases", type=int, default=1000)
    ap.add_argument("--mb", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("acc",), default=None)
    ap.add_argument("--streamed-only", action="store_true",
                    help="command: leave the whole path out (larger files than it has memory for); stored as `command_streamed_only`")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--tmp-dir", default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "sketch_sample"))
    ap.add_argument("--no-merge", action="store_true", help="print the leg's result only (a traced run)")
    args = ap.parse_args()
    if args.leg != "trace" and _lib.device_count() < 1:
        raise SystemExit("bench_sketch_sample.py needs a HIP device: nothing is measured without one")
    res = {"device": leg_device, "command": leg_command, "trace": leg_trace}[args.leg](args)
    print(json.dumps(res))
    if args.no_merge:
        return
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "bench_sketch_sample.json")
    doc = {"device": "unmeasured", "trace": "unmeasured", "command": "unmeasured"}
    if os.path.exists(path):
        with open(path) as f:
            doc.update(json.load(f))
    doc["command_streamed_only" if args.leg == "command" and args.streamed_only else args.leg] = res
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
