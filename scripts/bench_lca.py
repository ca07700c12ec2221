#!/usr/bin/env python3
"""Device time of the lineage pass (yh_lca_device) next to the passes that make the same reads, and what its taxonomy costs.

    python scripts/bench_lca.py [--n-refs 85205] [--iters 200] [--warmup 30] [--rounds 3] [--out FILE]

On the synthetic database at GTDB rs214 scale (synth.config3_device) with a synthetic taxonomy of depth 8 and about 1.3 nodes
per reference (synthetic_lineages below: how clusters map to genera), and for two sample shapes -- a 10^6-hash sample and a
real-shape 83 k-hash sample (synth.sample_device) -- these calls are timed in the same process, on the same samples and the
same abundances: yh_lca_device counts-only (d_node = NULL) and with nodes, yh_lca_device counts-only without abundances,
yh_explain_device totals-only, and yh_abund_device sums-only, the yardstick: the same probe and the same LDS table, with a
posting-list walk where this pass has one 4-byte read.  HIP events on the handle's stream around `iters` back-to-back calls
that rotate through eight samples, after a warm-up of every call; the calls alternate inside each of `rounds` rounds and the
median round is reported with the spread.  Also recorded: the host wall time of yh_db_set_taxonomy, k_lca_index's own event
time (the library prints it to stderr with YH_DEBUG_TUNING=1 YH_TRACE_LCA=1, which this script sets and reads back) and the
longest posting list of the database.

Before anything is timed, the device's nodes and counts of the first sample of each shape must equal an oracle's that shares
nothing with the kernels: all (hash, reference) pairs sorted by torch, the holders of a sample hash found by searchsorted, and
the LCA taken as the longest common prefix of the holders' ancestor PATHS (a table of every node's ancestor at every depth;
per depth a segment minimum and maximum) -- no depth lifting.  Prints one JSON line and writes it to --out (default
profiles/lca/bench_lca.json).

    python scripts/bench_lca.py --batch [--batch-iters 10] [--batch-warmup 3] [--rounds 3] [--out FILE]

The batched leg alone (default --out profiles/lca/bench_lca_batch.json), on the same database and taxonomy: blocks of 256
real-shape 83 k-hash samples and of 32 samples of 10^6 hashes, resident on the device with their abundances.  Timed, alternating
inside each round: (a) one yh_lca_batch_device plus yh_lca_rows_pack_device, (b) a loop of yh_lca_device over the block's
samples, (c) the batched call without the pack -- HIP events, us per sample, the median of the rounds with their spread.  Before
anything is timed the block's dense counts must equal the loop's and the rows torch.nonzero of them, in order."""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

os.environ.setdefault("YH_DEBUG_TUNING", "1")
os.environ.setdefault("YH_TRACE_LCA", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yacht_amd import _lib, synth, taxonomy  # noqa: E402
from yacht_amd.engine import RefDB  # noqa: E402

N_ROTATE = 8
NONE = _lib.YH_LCA_NONE
MAPPING = ("a cluster of the synthetic database (a founder and the 1-7 references that copy 10-95 % of its hashes) is ONE genus: its "
           "members pair up into species, the first of a pair named at the species, the second a strain under it (depth 8); a "
           "reference outside every cluster is a species of its own, four consecutive ones to a genus; four genera to a family, "
           "four families to an order, and so on up to the superkingdoms")


def synthetic_lineages(founder: np.ndarray):
    """One lineage per reference from the cluster founders (synth.global_db_plan's `parent`): MAPPING."""
    n = founder.size
    genus_of = np.zeros(n, dtype=np.int64)
    g = -1
    singles = 0
    for j in range(n):
        clustered = founder[j] != j or (j + 1 < n and founder[j + 1] == j)
        if clustered:
            if founder[j] == j:
                g += 1
                singles = 0
            genus_of[j] = g
        else:
            if singles % 4 == 0:
                g += 1
            singles += 1
            genus_of[j] = g
    lineages = {}
    for j in range(n):
        g = int(genus_of[j])
        upper = (f"k{g // 4096:02d}", f"p{g // 1024:03d}", f"c{g // 256:04d}", f"o{g // 64:05d}", f"f{g // 16:05d}", f"g{g:06d}")
        k = j - int(founder[j])  # place in the cluster (0 outside one)
        clustered = founder[j] != j or (j + 1 < n and founder[j + 1] == j)
        species = f"g{g:06d}s{k // 2:02d}" if clustered else f"g{g:06d}r{j:06d}"
        lineages[f"r{j}"] = upper + ((species,) if not clustered or k % 2 == 0 else (species, f"{species}t"))
    return lineages


def torch_oracle(values, offsets, parent, depth, leaf, sample, abund):
    """(nodes int64 [n] with NONE for an absent hash, counts int64 [n_nodes, 2]) by sort, searchsorted and ancestor paths."""
    import torch

    dev = values.device
    n_refs, n_nodes = int(offsets.numel() - 1), int(parent.numel())
    sv, perm = torch.sort(values)
    sr = torch.repeat_interleave(torch.arange(n_refs, device=dev, dtype=torch.int64), offsets[1:] - offsets[:-1])[perm]
    del perm
    runs = torch.unique_consecutive(sv, return_counts=True)[1]
    longest = int(runs.max())
    del runs
    lo, hi = torch.searchsorted(sv, sample), torch.searchsorted(sv, sample, right=True)
    cnt = hi - lo
    n = int(sample.numel())
    seg = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int64), cnt)
    first = torch.cumsum(cnt, 0) - cnt
    holder = sr[lo[seg] + (torch.arange(int(seg.numel()), device=dev, dtype=torch.int64) - first[seg])]
    del sv, sr
    levels = int(depth.max()) + 1
    path = torch.full((n_nodes, levels), -1, dtype=torch.int64, device=dev)  # path[v][d] = v's ancestor at depth d
    cur = torch.arange(n_nodes, device=dev, dtype=torch.int64)
    for _ in range(levels):
        path[torch.arange(n_nodes, device=dev), depth[cur]] = cur
        cur = parent[cur]
    at = path[leaf[holder]]  # [entries, levels]
    agree = torch.ones(n, dtype=torch.bool, device=dev)
    nodes = torch.zeros(n, dtype=torch.int64, device=dev)
    for d in range(levels):
        lo_d = torch.full((n,), n_nodes, dtype=torch.int64, device=dev).scatter_reduce_(0, seg, at[:, d], "amin")
        hi_d = torch.full((n,), -2, dtype=torch.int64, device=dev).scatter_reduce_(0, seg, at[:, d], "amax")
        agree &= (lo_d == hi_d) & (lo_d >= 0)
        nodes = torch.where(agree, lo_d, nodes)
    known = cnt > 0
    nodes = torch.where(known, nodes, torch.full_like(nodes, NONE))
    counts = torch.zeros((n_nodes, 2), dtype=torch.int64, device=dev)
    counts[:, 0] = torch.bincount(nodes[known], minlength=n_nodes)
    counts[:, 1].scatter_add_(0, nodes[known], abund[known].long())
    return nodes, counts, longest, int((cnt >= 2).sum())


def timed_set_taxonomy(db, tree):
    """(host wall seconds of yh_db_set_taxonomy, k_lca_index's event time in ms or None) with the library's stderr read back."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            db.set_taxonomy(*tree)
            wall = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    sys.stderr.write(text)
    m = re.search(r"k_lca_index over (\d+) shared hashes took ([0-9.]+) ms", text)
    return wall, (float(m.group(2)) if m else None)


def batch_leg(args) -> dict:
    """(a) one yh_lca_batch_device plus yh_lca_rows_pack_device against (b) a loop of yh_lca_device over the same resident
    block, us per sample; the batched call alone is recorded beside them.  Equality with the loop -- every dense count, and
    the rows against torch.nonzero of them -- is checked before anything is timed."""
    import torch

    dev = torch.device("cuda:0")
    N = args.n_refs
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    plan = synth.global_db_plan(1002, N)
    assert np.array_equal(plan["offsets"], offsets.cpu().numpy())
    tree = taxonomy.build_tree([f"r{j}" for j in range(N)], synthetic_lineages(plan["parent"]))
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    db.set_taxonomy(*tree[:3])
    n_nodes = db.taxonomy_info()["n_nodes"]
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    result = {"bench": "lca_batch", "commit": args.commit, "n_refs": N, "n_hashes_db": int(values.numel()), "n_nodes": n_nodes,
              "iters": args.batch_iters, "warmup": args.batch_warmup, "rounds": args.rounds, "tile": _lib.YH_LCA_BATCH_TILE,
              "counts_bytes_per_sample": 16 * n_nodes, "shapes": {}}
    for name, shape, n_sample, b in (("real_shape_83k_x256", "real", 83_000, 256), ("1e6_hash_x32", "present", 1_000_000, 32)):
        samples = [synth.sample_device(values, offsets, seed=2900 + i, n_sample=n_sample, shape=shape) for i in range(b)]
        offs = np.zeros(b + 1, dtype=np.int64)
        offs[1:] = np.cumsum([int(s.numel()) for s in samples])
        total = int(offs[-1])
        d_samples = torch.cat(samples)
        del samples
        d_offs = torch.from_numpy(offs).to(dev)
        d_abund = torch.randint(1, 1001, (total,), generator=g, device=dev, dtype=torch.int32)
        counts = [torch.zeros((b, n_nodes, 2), dtype=torch.int64, device=dev) for _ in range(2)]
        cap = b * 32768  # (a real-shape sample meets ~21 000 nodes, a 10^6-hash one ~200: fewer than that, checked below)
        rows = torch.zeros((cap, 3), dtype=torch.int64, device=dev)
        n_rows = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def batched_alone():
            db.lca_batch_device(d_samples.data_ptr(), d_offs.data_ptr(), d_abund.data_ptr(), b, total, 0, counts[0].data_ptr())

        def batched():
            batched_alone()
            db.lca_rows_pack_device(counts[0].data_ptr(), b, rows.data_ptr(), cap, n_rows.data_ptr())

        def looped():
            for s in range(b):
                o = int(offs[s])
                db.lca_device(d_samples.data_ptr() + 8 * o, d_abund.data_ptr() + 4 * o, int(offs[s + 1]) - o, 0, counts[1][s].data_ptr())

        batched()
        looped()
        db.synchronize()
        assert torch.equal(counts[0], counts[1]) and int(counts[0][:, :, 0].sum(dim=1).min()) > 0, "the block differs from the loop"
        k = int(n_rows[0])
        at = torch.nonzero(counts[1][:, :, 0])  # row-major: ascending (sample, node)
        assert k == int(at.shape[0]) <= cap, "the row count differs from the loop's non-zero cells"
        view = rows[:k].cpu().numpy().reshape(-1).view(np.dtype([("sample", np.uint32), ("node", np.uint32), ("n", np.uint64), ("w", np.uint64)]))
        picked = counts[1][at[:, 0], at[:, 1]].cpu().numpy()
        at = at.cpu().numpy()
        assert np.array_equal(view["sample"], at[:, 0]) and np.array_equal(view["node"], at[:, 1]), "the rows' order differs"
        assert np.array_equal(view["n"].astype(np.int64), picked[:, 0]) and np.array_equal(view["w"].astype(np.int64), picked[:, 1])
        calls = (("batched_us_per_sample", batched), ("looped_us_per_sample", looped), ("batched_without_pack_us_per_sample", batched_alone))
        times = {k_: [] for k_, _ in calls}
        with torch.cuda.stream(stream):
            for _k, fn in calls:
                for _ in range(args.batch_warmup):
                    fn()
            db.synchronize()
            for _ in range(args.rounds):
                for k_, fn in calls:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _i in range(args.batch_iters):
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    times[k_].append(e0.elapsed_time(e1) * 1e3 / args.batch_iters / b)
        out = {"samples": b, "total_hashes": total, "hashes_in_database": int(counts[0][:, :, 0].sum()), "rows": k,
               "rows_per_sample_mean": round(k / b, 1), "counts_bytes": 16 * b * n_nodes,
               "equal": "every dense count equals the loop's; the rows equal torch.nonzero of them in (sample, node) order"}
        for k_, v in times.items():
            out[k_] = round(float(np.median(v)), 2)
            out[k_.replace("_us_per_sample", "_rounds_us_per_sample")] = [round(x, 2) for x in v]
            out[k_.replace("_us_per_sample", "_spread_us_per_sample")] = round(max(v) - min(v), 2)
        spread = max(out["batched_spread_us_per_sample"], out["looped_spread_us_per_sample"])
        out["batched_over_looped"] = round(out["batched_us_per_sample"] / out["looped_us_per_sample"], 3)
        # the expectation: batched plus pack no longer than the loop, judged against the rounds' spread
        out["batched_not_slower"] = bool(out["batched_us_per_sample"] <= out["looped_us_per_sample"] + spread)
        result["shapes"][name] = out
        del d_samples, d_abund, counts, rows
        torch.cuda.empty_cache()
    db.close()
    return result


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="store_true", help="the batched leg alone (yh_lca_batch_device + rows pack against a loop of yh_lca_device)")
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
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lca",
                                "bench_lca_batch.json" if args.batch else "bench_lca.json")
    import torch

    assert _lib.device_count() >= 1, "bench_lca.py needs an MI355X"
    if args.batch:
        line = json.dumps(batch_leg(args))
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return
    dev = torch.device("cuda:0")
    N = args.n_refs
    values, offsets, _ = synth.config3_device(seed=1002, n_refs=N, n_sample=1000, device="cuda:0")
    torch.cuda.synchronize()
    plan = synth.global_db_plan(1002, N)
    assert np.array_equal(plan["offsets"], offsets.cpu().numpy())  # (the same random stream: the plan's founders are the database's)
    t0 = time.perf_counter()
    tree = taxonomy.build_tree([f"r{j}" for j in range(N)], synthetic_lineages(plan["parent"]))
    build_tree_s = time.perf_counter() - t0
    parent, depth, leaf = tree[:3]
    assert tree[4] == 0 and int(depth.max()) == 8
    db = RefDB.from_device(values.data_ptr(), offsets.data_ptr(), N)
    stream = torch.cuda.Stream()
    db.set_stream(stream.cuda_stream)
    walls, index_ms = [], []
    for _ in range(3):
        wall, ms = timed_set_taxonomy(db, (parent, depth, leaf))
        walls.append(wall)
        index_ms.append(ms)
    info = db.info()
    tax = db.taxonomy_info()
    n_nodes = tax["n_nodes"]
    t_parent, t_depth, t_leaf = (torch.from_numpy(a.astype(np.int64)).to(dev) for a in (parent, depth, leaf))
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    result = {"bench": "lca", "n_refs": N, "n_hashes_db": int(values.numel()), "iters": args.iters, "warmup": args.warmup,
              "rounds": args.rounds, "samples_rotated": N_ROTATE,
              "taxonomy": {"n_nodes": n_nodes, "nodes_per_reference": round(n_nodes / N, 3), "depth": int(depth.max()),
                           "device_bytes": tax["device_bytes"], "clusters_to_genera": MAPPING,
                           "references_in_clusters": int(sum(1 for j in range(N) if plan["parent"][j] != j or (j + 1 < N and plan["parent"][j + 1] == j))),
                           "build_tree_host_s": round(build_tree_s, 3)},
              "set_taxonomy_host_wall_ms": [round(w * 1e3, 3) for w in walls],
              "set_taxonomy_host_wall_ms_median": round(float(np.median(walls)) * 1e3, 3),
              "k_lca_index_event_ms": index_ms,
              "k_lca_index_event_ms_median": None if any(m is None for m in index_ms) else round(float(np.median(index_ms)), 3),
              "k_lca_index_form": "one lane per shared hash, leaving a list once the fold is the root",
              "n_shared_distinct": int(info["n_shared_distinct"]), "n_shared_postings": int(info["n_shared_postings"]), "shapes": {}}
    for name, shape, n_sample in (("1e6_hash", "present", 1_000_000), ("real_shape_83k", "real", 83_000)):
        samples = [synth.sample_device(values, offsets, seed=900 + i, n_sample=n_sample, shape=shape) for i in range(N_ROTATE)]
        abunds = [torch.randint(1, 1001, (int(s.numel()),), generator=g, device=dev, dtype=torch.int32) for s in samples]
        nodes = torch.zeros(max(int(s.numel()) for s in samples), dtype=torch.int32, device=dev)
        counts = torch.zeros((n_nodes, 2), dtype=torch.int64, device=dev)
        totals = torch.zeros(16, dtype=torch.int64, device=dev)
        w_ov = torch.zeros(N, dtype=torch.int64, device=dev)
        w_m = torch.zeros(N, dtype=torch.int64, device=dev)
        member = torch.ones(N, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def lca_counts(i):
            db.lca_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), 0, counts.data_ptr())

        def lca_nodes(i):
            db.lca_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), nodes.data_ptr(), counts.data_ptr())

        def lca_counts_flat(i):
            db.lca_device(samples[i].data_ptr(), 0, int(samples[i].numel()), 0, counts.data_ptr())

        def explain_totals(i):
            db.explain_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), member.data_ptr(), 0, totals.data_ptr())

        def abund_sums(i):
            db.abundance_device(samples[i].data_ptr(), abunds[i].data_ptr(), int(samples[i].numel()), w_ov.data_ptr(), w_m.data_ptr(), 0)

        # the device against the oracle, before anything is timed: every node word and both columns of the counts
        want_nodes, want_counts, longest, n_shared_hits = torch_oracle(values, offsets, t_parent, t_depth, t_leaf, samples[0], abunds[0])
        lca_nodes(0)
        db.synchronize()
        n0 = int(samples[0].numel())
        assert torch.equal(nodes[:n0].long() & 0xFFFFFFFF, want_nodes), "nodes differ from the oracle's"
        assert torch.equal(counts, want_counts), "counts differ from the oracle's"
        lca_counts(0)
        db.synchronize()
        assert torch.equal(counts, want_counts), "counts-only differs from the oracle's"
        lca_counts_flat(0)
        db.synchronize()
        assert torch.equal(counts[:, 0], want_counts[:, 0]) and torch.equal(counts[:, 1], counts[:, 0])
        explain_totals(0)
        db.synchronize()
        assert int(totals[14]) == int(want_counts[:, 0].sum()) and int(totals[15]) == int(want_counts[:, 1].sum())
        result["longest_posting_list"] = longest
        shared = want_nodes[(want_nodes != NONE)]
        calls = (("lca_counts_only_us", lca_counts), ("lca_with_nodes_us", lca_nodes), ("lca_counts_only_no_abund_us", lca_counts_flat),
                 ("explain_totals_only_us", explain_totals), ("abund_sums_only_us", abund_sums))
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
        out = {"n_sample": n0, "hashes_in_database": int(want_counts[:, 0].sum()), "hashes_shared": n_shared_hits,
               "nodes_hit": int((want_counts[:, 0] > 0).sum()), "hashes_at_depth": torch.bincount(t_depth[shared], minlength=9).tolist(),
               "oracle": "equal: every node word, both columns of the counts, counts-only, and without abundances"}
        for k, v in times.items():
            out[k] = round(float(np.median(v)), 2)
            out[k.replace("_us", "_rounds_us")] = [round(x, 2) for x in v]
        spreads = [max(times[k]) - min(times[k]) for k in ("lca_counts_only_us", "abund_sums_only_us")]
        margin = max(0.10 * out["abund_sums_only_us"], max(spreads))
        out["margin_us"] = round(margin, 2)
        for k in ("lca_counts_only_us", "lca_with_nodes_us", "lca_counts_only_no_abund_us"):
            out[k.replace("_us", "_over_abund_sums")] = round(out[k] / out["abund_sums_only_us"], 3)
        # the expectation: no longer than the sums-only abundance pass, judged with 10 % or the rounds' spread, whichever is larger
        out["lca_counts_only_not_slower_than_abund_sums"] = bool(out["lca_counts_only_us"] <= out["abund_sums_only_us"] + margin)
        out["lca_with_nodes_not_slower_than_abund_sums"] = bool(out["lca_with_nodes_us"] <= out["abund_sums_only_us"] + margin)
        result["shapes"][name] = out
        del samples, abunds
    db.close()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
