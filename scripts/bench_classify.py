#!/usr/bin/env python3
"""Device time of the per-record classification (yh_classify_sets_device) next to the unchanged yh_lca_device with nodes on the
same number of hashes, and the two legs around it.

    python scripts/bench_classify.py [--legs sets,sketch,command] [--n-refs 85205] [--iters 50] [--rounds 3] [--out FILE]

Leg `sets`.  On the synthetic database at GTDB rs214 scale with the synthetic taxonomy of scripts/bench_lca.py.  The hashes of a
shape are ONE real-shape sample of that many hashes (synth.sample_device(shape="real"), the device form of the draw
bench_cohort.py makes), dealt at random to the sets and sorted inside each set.  That draw holds about 77 000 database hashes
WHATEVER its size, the rest is noise: about 30 % of the entries of the read and long-read shapes are in the database and 3 % of
the bins' (the JSON gives `hits` per shape), so the shapes are mostly misses that the presence filter turns away, on both sides
of the comparison.  Three shapes: reads (1.7 x 10^6 sets, 2.6 x 10^5 entries in all: most sets are empty), long reads (2.7 x 10^4
sets of about 10), bins (512 sets of 5 000).  The yardstick is yh_lca_device with d_node on the same hashes as one sorted distinct
sample: the same probe and the same dependent read, the hit table in place of the fold.  yh_classify_sets_device is timed
twice, with d_node (like for like) and without.  HIP events on the handle's stream around `iters` back-to-back calls after one
warm call; the calls alternate inside each of `rounds` rounds; the median round is reported with min - max.  Before anything is
timed, every node word must equal a torch oracle's (bench_lca.torch_oracle) and the rows of the first 2 000 non-empty sets a
numpy fold over ancestor paths.

Leg `sketch`.  --sketch-mib (256) MiB of seeded random 150-base reads resident in HBM, one segment per read:
yh_sketch_segments_device alone against the same call followed by yh_classify_sets_device on the CSR it leaves, both on the
handle's stream, same clock.  `total` is read back once (the call needs the host's copy); random reads hit nothing in the
database, which the JSON states: the lookup's filter turns nearly every entry away.

Leg `command`.  Host clock: `yacht classify` (classify.main, with its phases) on a written FASTA of --contigs (10^5) random contigs
of 2 to 4 kb against a database and lineage table as bench_cohort.py makes them, then YACHT_CLASSIFY=loop on the first
--loop-contigs (2 000) of them.  Random contigs hit nothing either.

A leg that is not run is "unmeasured" in the JSON.  Prints one JSON line and writes it to --out (default
profiles/classify/bench_classify.json)."""
from __future__ import annotations

import argparse
import json
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import bench_lca  # noqa: E402
from yacht_amd import _lib, sketch, synth, taxonomy  # noqa: E402
from yacht_amd.engine import CLASSIFY_ROW_DTYPE, RefDB  # noqa: E402

NONE = _lib.YH_LCA_NONE
SHAPES = (("reads", 1_700_000, 260_000, "random"), ("long_reads", 27_000, 270_000, "random"), ("bins", 512, 512 * 5000, "equal"))


def deal(torch, sample, n_sets, how, seed):
    """(mins, off): the sorted distinct `sample` dealt to n_sets sets, ascending inside each set."""
    dev = sample.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n = int(sample.numel())
    if how == "equal":
        ids = torch.arange(n, device=dev) % n_sets
        ids = ids[torch.randperm(n, generator=g, device=dev)]
    else:
        ids = torch.randint(0, n_sets, (n,), generator=g, device=dev)
    order = torch.sort(ids, stable=True)[1]  # (the sample ascends: a stable sort by set keeps every set ascending)
    off = torch.zeros(n_sets + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(torch.bincount(ids, minlength=n_sets), 0)
    return sample[order].contiguous(), off


def numpy_rows(parent, depth, nodes, off, sets):
    """rows of the given sets from per-entry nodes: the LCA as the deepest level at which all ancestor paths agree."""
    levels = int(depth.max()) + 1
    path = np.full((parent.size, levels), -1, dtype=np.int64)
    cur = np.arange(parent.size)
    for _ in range(levels):
        path[np.arange(parent.size), depth[cur]] = cur
        cur = parent[cur]
    rows = np.zeros(len(sets), dtype=CLASSIFY_ROW_DTYPE)
    for i, s in enumerate(sets):
        mine = nodes[off[s]:off[s + 1]]
        hit = mine[mine != NONE]
        inf = np.unique(hit[hit != 0])
        node = NONE if hit.size == 0 else 0
        if inf.size:
            p = path[inf]
            agree = (p == p[0]).all(axis=0) & (p[0] >= 0)
            node = int(p[0][np.flatnonzero(np.cumprod(agree))[-1]])
        rows[i] = (node, mine.size, hit.size, int((hit == 0).sum()))
    return rows


def leg_sets(args, torch) -> dict:
    dev = torch.device("cuda:0")
    N = args.n_refs
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    plan = synth.global_db_plan(1002, N)
    tree = taxonomy.build_tree([f"r{j}" for j in range(N)], bench_lca.synthetic_lineages(plan["parent"]))
    parent, depth, leaf = tree[:3]
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    db.set_taxonomy(parent, depth, leaf)
    n_nodes = db.taxonomy_info()["n_nodes"]
    t_parent, t_depth, t_leaf = (torch.from_numpy(a.astype(np.int64)).to(dev) for a in (parent, depth, leaf))
    out = {"n_refs": N, "n_nodes": n_nodes, "iters": args.iters, "rounds": args.rounds, "warm_calls": 1, "measured": True,
           "yardstick": "yh_lca_device with d_node on the same hashes as one sorted distinct sample", "shapes": {}}
    for k, (name, n_sets, n_entries, how) in enumerate(SHAPES):
        sample = synth.sample_device(values, offsets, seed=700 + k, n_sample=n_entries, shape="real")
        total = int(sample.numel())
        mins, off = deal(torch, sample, n_sets, how, 31 + k)
        rows = torch.zeros(4 * n_sets, dtype=torch.int32, device=dev)
        node = torch.zeros(total, dtype=torch.int32, device=dev)
        node_l = torch.zeros(total, dtype=torch.int32, device=dev)
        counts = torch.zeros((n_nodes, 2), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def classify(with_nodes=False):
            db.classify_sets_device(mins.data_ptr(), off.data_ptr(), n_sets, total, rows.data_ptr(), node.data_ptr() if with_nodes else 0)

        def lca():
            db.lca_device(sample.data_ptr(), 0, total, node_l.data_ptr(), counts.data_ptr())

        ones = torch.ones(total, dtype=torch.int32, device=dev)
        want_nodes = bench_lca.torch_oracle(values, offsets, t_parent, t_depth, t_leaf, mins, ones)[0]
        classify(True)
        db.synchronize()
        assert torch.equal(node.long() & 0xFFFFFFFF, want_nodes), "nodes differ from the oracle's"
        h_off = off.cpu().numpy()
        some = np.flatnonzero(np.diff(h_off) > 0)[:2000]
        got = rows.cpu().numpy().view(CLASSIFY_ROW_DTYPE)
        want = numpy_rows(parent.astype(np.int64), depth.astype(np.int64), want_nodes.cpu().numpy(), h_off, some.tolist())
        assert got[some].tobytes() == want.tobytes(), "rows differ from the oracle's"
        empty = np.flatnonzero(np.diff(h_off) == 0)
        assert (got["node"][empty] == NONE).all() and (got["n_kept"][empty] == 0).all()
        calls = (("classify_sets_with_nodes_us", lambda: classify(True)), ("classify_sets_rows_only_us", classify), ("lca_with_nodes_us", lca))
        times = time_calls(torch, db, stream, calls, args.iters, args.rounds)
        shape = {"n_sets": n_sets, "entries": total, "hits": int((want_nodes != NONE).sum()), "empty_sets": int(empty.size)}
        shape.update(times)
        a, b = shape["classify_sets_with_nodes_us"], shape["lca_with_nodes_us"]
        spread = max(a["max"] - a["min"], b["max"] - b["min"])
        shape["ratio_to_yardstick"] = round(a["median"] / b["median"], 3)
        shape["no_slower_at_larger_of_10pct_and_spread"] = bool(a["median"] <= b["median"] + max(0.1 * b["median"], spread))
        out["shapes"][name] = shape
        del sample, mins, off, rows, node, node_l, counts, ones, want_nodes
    db.close()
    return out


def time_calls(torch, db, stream, calls, iters, rounds) -> dict:
    """{name: {median, min, max}} in us per call: one warm call each, then `rounds` rounds in which the calls alternate."""
    times = {c: [] for c, _ in calls}
    with torch.cuda.stream(stream):
        for _c, fn in calls:
            fn()
        db.synchronize()
        for _ in range(rounds):
            for c, fn in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _i in range(iters):
                    fn()
                e1.record(stream)
                e1.synchronize()
                times[c].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {c: {"median": round(float(np.median(t)), 2), "min": round(min(t), 2), "max": round(max(t), 2)} for c, t in times.items()}


def leg_sketch(args, torch) -> dict:
    """yh_sketch_segments_device alone against sketch + classify on resident random 150-base reads."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    N = args.n_refs
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    plan = synth.global_db_plan(1002, N)
    parent, depth, leaf = taxonomy.build_tree([f"r{j}" for j in range(N)], bench_lca.synthetic_lineages(plan["parent"]))[:3]
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    db.set_taxonomy(parent, depth, leaf)
    n = args.sketch_mib << 20
    gen = torch.Generator(device="cuda").manual_seed(9)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n,), generator=gen, device=dev)]
    seg = torch.arange(0, n + 150, 150, dtype=torch.int64, device=dev).clamp_(max=n)
    n_seg = int(seg.numel()) - 1
    k, mh = 31, sketch.max_hash_for_scaled(1000)
    cap = int(n / 1000 * 1.25) + 4096
    wb = int(lib.yh_sketch_segments_work_bytes(cap, n_seg))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    mins = torch.empty(cap, dtype=torch.int64, device=dev)
    abund = torch.empty(cap, dtype=torch.int32, device=dev)
    off = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    rows = torch.zeros(4 * n_seg, dtype=torch.int32, device=dev)
    st = C.c_void_p(stream.cuda_stream)

    def sk():
        _lib.check(lib.yh_sketch_segments_device(C.c_void_p(seq.data_ptr()), n, C.c_void_p(seg.data_ptr()), n_seg, k, 42, mh, cap,
                                                 C.c_void_p(work.data_ptr()), wb, cap, C.c_void_p(mins.data_ptr()), C.c_void_p(abund.data_ptr()),
                                                 C.c_void_p(off.data_ptr()), C.c_void_p(totals.data_ptr()), st))

    torch.cuda.synchronize()  # (the reads were drawn on another stream)
    with torch.cuda.stream(stream):
        sk()
    db.synchronize()
    kept, total = (int(x) for x in totals.cpu())
    assert 0 < kept <= cap and int(off[-1].item()) == total

    def both():
        sk()
        db.classify_sets_device(mins.data_ptr(), off.data_ptr(), n_seg, total, rows.data_ptr(), 0)

    both()
    db.synchronize()
    got = rows.cpu().numpy().view(CLASSIFY_ROW_DTYPE)
    assert np.array_equal(got["n_kept"], np.diff(off.cpu().numpy()).astype(np.uint32))
    out = {"measured": True, "bytes": n, "reads": n_seg, "kept_hashes": total, "hits": int(got["n_hit"].sum(dtype=np.uint64)),
           "note": "seeded random reads: they hit nothing in the database, so the lookup's filter turns nearly every entry away",
           "iters": args.sketch_iters, "rounds": args.rounds}
    out.update(time_calls(torch, db, stream, (("sketch_segments_us", sk), ("sketch_plus_classify_us", both)), args.sketch_iters, args.rounds))
    out["classify_adds_us"] = round(out["sketch_plus_classify_us"]["median"] - out["sketch_segments_us"]["median"], 2)
    db.close()
    return out


def leg_command(args) -> dict:
    """`yacht classify` on a written FASTA against YACHT_CLASSIFY=loop on its first records, host clock, with the phases."""
    import bench_cohort
    from types import SimpleNamespace

    from yacht_amd import classify, phases

    out = {"measured": True, "clock": "host perf_counter", "contigs": args.contigs, "loop_contigs": args.loop_contigs,
           "note": "random contigs of 2 to 4 kb: they hit nothing in the database"}
    with tempfile.TemporaryDirectory() as tmp:
        cfg, _v, _o = bench_cohort.make_db(tmp, args.n_refs, 1002)
        lin = bench_cohort.make_lineages(tmp, args.n_refs)
        rng = np.random.default_rng(3)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        paths = {}
        for name, count in (("all", args.contigs), ("first", args.loop_contigs)):
            rng = np.random.default_rng(3)  # (the same records from the start)
            paths[name] = os.path.join(tmp, f"contigs_{name}.fa")
            with open(paths[name], "wb") as f:
                for i in range(count):
                    s = acgt[rng.integers(0, 4, int(rng.integers(2000, 4001)))].tobytes()
                    f.write(b">contig_%d\n" % i + b"\n".join(s[j:j + 80] for j in range(0, len(s), 80)) + b"\n")
        out["fasta_bytes"] = os.path.getsize(paths["all"])
        for key, which, env in (("device_route", "all", None), ("device_route_first", "first", None), ("loop_route_first", "first", "loop")):
            os.environ.pop(classify.ROUTE_ENV, None)
            if env:
                os.environ[classify.ROUTE_ENV] = env
            phases.reset()
            t0 = time.perf_counter()
            classify.main(SimpleNamespace(json=cfg, lineages=lin, infile=[paths[which]], outdir=os.path.join(tmp, key), min_hits=2, num_threads=16))
            out[key] = {"wall_s": round(time.perf_counter() - t0, 3), "phases": phases.snapshot()}
        os.environ.pop(classify.ROUTE_ENV, None)
        a = open(os.path.join(tmp, "device_route_first", "results", classify.RECORDS_NAME), "rb").read()
        assert a == open(os.path.join(tmp, "loop_route_first", "results", classify.RECORDS_NAME), "rb").read(), "the routes' files differ"
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="sets,sketch,command", help="comma-separated: sets, sketch, command; a leg left out is 'unmeasured'")
    ap.add_argument("--n-refs", type=int, default=85_205)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sketch-mib", type=int, default=256)
    ap.add_argument("--sketch-iters", type=int, default=5)
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--loop-contigs", type=int, default=2_000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "classify", "bench_classify.json"))
    args = ap.parse_args()
    legs = [w for w in args.legs.split(",") if w]
    assert set(legs) <= {"sets", "sketch", "command"}, legs
    import torch

    assert _lib.device_count() >= 1, "bench_classify.py needs an MI355X"
    result = {"bench": "classify", "sets": "unmeasured", "sketch_plus_classify_resident_reads": "unmeasured",
              "yacht_classify_vs_loop_host_clock": "unmeasured", "kernel_trace": "profiles/classify/kernel_stats.txt"}
    if "sets" in legs:
        result["sets"] = leg_sets(args, torch)
    if "sketch" in legs:
        result["sketch_plus_classify_resident_reads"] = leg_sketch(args, torch)
    if "command" in legs:
        result["yacht_classify_vs_loop_host_clock"] = leg_command(args)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
