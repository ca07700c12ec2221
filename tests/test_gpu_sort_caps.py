"""The build's distribution sort ON its capacities: a bucket of 4 095 / 4 096 / 4 097 pairs, a slot of 1 023 / 1 024 / 1 025,
a first-level region over cap1 -- and the side list that takes what exceeds them, wherever the bucket sits.

tests/sort_cap_cases.py builds the databases and holds a numpy model of the one linear function the sort cuts everything from;
tests/test_sort_cap_cases_cpu.py asserts that every case is what its name says.  Here every case is built on the device as
`yacht train`'s handle (YH_DB_PAIRWISE_ONLY), a full handle and a YH_DB_NO_INDEX handle, from host arrays and -- unchunked
rows -- from device arrays, and everything is compared by integer equality:
  * which way the database went: info()["sort_path"], the ONE verdict line of YH_TRACE_BUILD ("taken" / "REFUSED", on a
    refusal the flag bit that names the capacity), n_spilled_buckets and n_spilled_pairs equal to the model's figures --
    zero in the "not spilled" cases;
  * the train handle: pairwise(0.5) and index_stats() against oracle.train_pairs, single rows at a low threshold (holders of
    every hot hash, of a 2-holder and a 9-holder hash of the target, a sketch outside it) against oracle.overlap of the row's
    own sketch, nshared_device against the full handle's;
  * the sorting handles: run_counts, overlap and exclusive against the oracle for a sample of the hot hashes, the targets'
    smallest and largest keys, their 1-, 2-, 5- and 9-holder hashes, the neighbours across the targets' edges, hashes of a hot
    hash's bucket and slot that nobody holds, and a few hundred uniform ones; YH_CHECK_SORT=1 has the device check the order
    of the sorted pairs whichever sort made them.
Rows (tuning variables are read at first use: child processes, one after another, at most a dozen builds each): the default
build; the two-level sort forced (no side list there: REFUSED, then rocPRIM, and still exact); YH_FZ_NO_INLINE=1, every
pairwise record in list form, so that records name lists on both sides of fz_list_split; the chunked upload, host form only,
where the train handle goes through the pieces chunk by chunk and the others through the two-level sort.

Not covered: the side list's own capacity, max(H / 16, 2^20) pairs, which databases this small cannot reach.
"""
import json
import os
import re
import subprocess
import sys

import pytest

import sort_cap_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRWISE_ONLY, NO_INDEX = 8, 1
C_LOW = 0.004

WORKER = r"""
import json, os, sys
import numpy as np
root, names, jobs, c_low = sys.argv[1], sys.argv[2].split(","), [j.split(":") for j in sys.argv[3].split(",")], float(sys.argv[4])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import sort_cap_cases as sc
from oracle import oracle
from yacht_amd.engine import RefDB, YH_DB_NO_INDEX, YH_DB_PAIRWISE_ONLY
torch = None
if any(form == "device" for _, form in jobs):
    import torch

def say(msg):
    sys.stderr.flush()
    print("[caps] " + msg, file=sys.stderr, flush=True)

def create(v, o, flags, form):
    if form == "host":
        return RefDB(v, o, flags=flags), None
    dv = torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).to("cuda:0")
    do = torch.from_numpy(np.ascontiguousarray(o).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return RefDB.from_device(dv.data_ptr(), do.data_ptr(), o.size - 1, flags=flags), (dv, do)

def nshared(db, n):
    if torch is not None:
        t = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        db.nshared_device(t.data_ptr())
        db.synchronize()
        return t.cpu().numpy().astype(np.uint32)
    return None

out = []
for step, name in enumerate(names):
    c = sc.case(name)
    values, offsets = np.array(c.values), np.array(c.offsets)
    sizes = np.diff(offsets.astype(np.int64))
    sample = c.sample()
    want_ov = oracle.overlap(values, offsets, sample, threads=4)
    want_e, want_m = oracle.exclusive(values, offsets, want_ov > 0, sample)
    wi, wj, wc, wstats = oracle.train_pairs(values, offsets, 0.5, threads=4)
    want_rows = {}
    for r in c.rows:   # the oracle's row r: |R_r & R_j| for every j, kept unless count / |R_r| < c
        ov = oracle.overlap(values, offsets, c.sketch(r), threads=4).astype(np.int64)
        ov[r] = 0
        keep = np.flatnonzero((ov > 0) & ~(1.0 * ov / max(int(sizes[r]), 1) < c_low))
        want_rows[r] = (keep.astype(np.uint32), ov[keep].astype(np.uint32))
    hot_seen = all(bool(np.all(want_ov[js] > 0)) for _, js in c.hot)
    res = {"name": name, "H": c.H, "n_refs": c.n_refs, "pairs": int(wi.size), "overlapping": int((want_ov > 0).sum()), "hot_seen": hot_seen,
           "row_pairs": [int(want_rows[r][0].size) for r in c.rows],
           "hot_row_pairs": [int(want_rows[r][0].size) for _, js in c.hot for r in (js[0], js[-1])], "builds": {}}
    ns_ref = None
    for flags, form in jobs:
        flags = int(flags)
        key = f"{step}:{flags}:{form}"
        say(f"begin {key}")
        db, keepalive = create(values, offsets, flags, form)
        say(f"end {key}")
        wrong = []
        with db:
            info = db.info()
            if flags & YH_DB_PAIRWISE_ONLY:
                gi, gj, gc = db.pairwise(0.5)
                if not (np.array_equal(gi, wi) and np.array_equal(gj, wj) and np.array_equal(gc, wc)):
                    wrong.append(f"pairwise(0.5): {gi.size} pairs, the oracle has {wi.size}")
                if db.index_stats() != wstats:
                    wrong.append(f"index_stats {db.index_stats()} != {wstats}")
                for r in c.rows:
                    ri, rj, rc = db.pairwise(c_low, r, r + 1)
                    if not (np.all(ri == r) and np.array_equal(rj, want_rows[r][0]) and np.array_equal(rc, want_rows[r][1])):
                        wrong.append(f"row {r}: {rj.size} pairs, the oracle has {want_rows[r][0].size}")
            elif flags & YH_DB_NO_INDEX:
                if not np.array_equal(db.overlap(sample), want_ov):
                    wrong.append("overlap differs from the oracle")
            else:
                ov, e, m = db.run_counts(sample)
                if not (np.array_equal(ov, want_ov) and np.array_equal(e, want_e) and np.array_equal(m, want_m)):
                    wrong.append("run_counts differ from the oracle")
                if not np.array_equal(db.overlap(sample), want_ov):
                    wrong.append("overlap differs from the oracle")
                e2, m2 = db.exclusive(want_ov > 0, sample)
                if not (np.array_equal(e2, want_e) and np.array_equal(m2, want_m)):
                    wrong.append("exclusive differs from the oracle")
            ns = None
            if not (flags & YH_DB_NO_INDEX):
                ns = nshared(db, c.n_refs)
                if ns is not None and not flags:
                    ns_ref = ns
        del keepalive
        res["builds"][f"{flags}:{form}"] = {"key": key, "wrong": wrong, "sort_path": int(info["sort_path"]), "n_spilled_buckets": int(info["n_spilled_buckets"]),
                                           "n_spilled_pairs": int(info["n_spilled_pairs"]), "nshared": None if ns is None else ns.tolist()}
    # nshared_device of every handle that has one equals the full handle's
    for b in res["builds"].values():
        ns = b.pop("nshared")
        if ns is not None and ns_ref is not None and not np.array_equal(np.asarray(ns, np.uint32), ns_ref):
            b["wrong"].append("nshared_device differs from the full handle's")
        b["nshared_compared"] = ns is not None and ns_ref is not None
    out.append(res)
print(json.dumps(out))
"""

FORCED_TWO_LEVEL = {"YH_NO_PIECES": "1", "YH_NO_PIECES_SORT": "1"}
CHUNKED = {"YH_UPLOAD_CHUNK_MIN": "1", "YH_UPLOAD_SHARES": "0.4,0.3,0.2,0.1"}
# row -> (environment, builds of every case as flags:form (the full handle first: the others' nshared is compared with its), cases per child)
ROWS = {
    "default": ({}, ["0:host", "8:host", "1:host", "0:device", "8:device", "1:device"], 2),
    "two_level": (FORCED_TWO_LEVEL, ["0:host", "8:host", "1:host", "0:device", "8:device", "1:device"], 2),
    # (the switch changes `yacht train`'s records and nothing else: its handle in both forms, the full handle for nshared_device)
    "no_inline": ({"YH_FZ_NO_INLINE": "1"}, ["0:device", "8:host", "8:device"], 4),
    "chunked": (CHUNKED, ["0:host", "8:host", "1:host"], 4),
}


def path_of(row, flags):
    """The distribution a build goes down: the pieces unless the row forbids them -- the chunked upload feeds every handle but
    `yacht train`'s to the two-level sort chunk by chunk."""
    if row == "two_level" or (row == "chunked" and not flags & PAIRWISE_ONLY):
        return "two_level"
    return "pieces"


def _groups():
    for row, (_, _, per_child) in ROWS.items():
        for k in range(0, len(sc.NAMES), per_child):
            yield pytest.param(row, sc.NAMES[k:k + per_child], id=f"{row}-{'+'.join(sc.NAMES[k:k + per_child])}")


def _run(names, jobs, env_extra):
    env = dict(os.environ)
    env.update({"YH_DEBUG_TUNING": "1", "YH_TRACE_BUILD": "1", "YH_CHECK_SORT": "1"})
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", WORKER, ROOT, ",".join(names), ",".join(jobs), repr(C_LOW)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), [ln.rstrip() for ln in r.stderr.splitlines()]


def _verdicts(lines, key):
    a, z = lines.index(f"[caps] begin {key}"), lines.index(f"[caps] end {key}")
    seg = lines[a + 1:z]
    return seg, [ln for ln in seg if (ln.startswith("[yh sort]") or ln.startswith("[yh pieces]")) and " -> " in ln]


def _check_build(row, name, flags, form, got, lines):
    c = sc.case(name)
    handle = "train" if flags & PAIRWISE_ONLY else "sort"
    path = path_of(row, flags)
    want = c.expected(handle, path)
    print(f"{row:9s} {name:17s} flags {flags} {form:6s} {path:9s}: sort_path {got['sort_path']} side list {got['n_spilled_buckets']} buckets "
          f"{got['n_spilled_pairs']} pairs (model: {want['sort_path']}, {want['n_spilled_buckets']}, {want['n_spilled_pairs']})  wrong {len(got['wrong'])}")
    where = (row, name, flags, form)
    # 1. the path and the side list, exact
    assert got["sort_path"] == want["sort_path"], where
    assert got["n_spilled_buckets"] == want["n_spilled_buckets"], where
    assert got["n_spilled_pairs"] == want["n_spilled_pairs"], where
    seg, verdicts = _verdicts(lines, got["key"])
    assert len(verdicts) == 1, (where, verdicts)
    v = verdicts[0]
    assert v.endswith("-> " + want["verdict"]), (where, v)
    printed = int(re.search(r"flags (\d+) ", v).group(1))
    if path == "pieces":
        assert v.startswith("[yh pieces]") and printed == 0, (where, v)
        p1, p2 = c.stated["pieces"]
        assert f"P1 {p1} x P2 {p2} = {p1 * p2} buckets" in v, (where, v)
        if handle == "sort":
            assert f" sorted {c.H} of {c.H}  side list {want['n_spilled_pairs']} pairs of {want['n_spilled_buckets']} buckets" in v, (where, v)
        else:
            assert f"records of {c.H} of {c.H}" in v, (where, v)
            side = [ln for ln in seg if ln.startswith("[yh pieces] side list:")]
            assert len(side) == (1 if want["n_spilled_pairs"] else 0), (where, side)
            if side:
                assert f"side list: {want['n_spilled_pairs']} pairs of {want['n_spilled_buckets']} overflowed buckets" in side[0], (where, side)
    else:
        p1, p2 = c.stated["two_level"]
        assert v.startswith("[yh sort]") and f"P1 {p1} x P2 {p2} = {p1 * p2} buckets  cap1 {sc.cap1_of(c.H, p1)} " in v, (where, v)
        assert ("fused: records of" if handle == "train" else " sorted ") in v, (where, v)
        if want["bit"]:
            assert printed & want["bit"], (where, v)          # the capacity that was exceeded is named
            if want["bit"] == 4:
                assert printed == 4, (where, v)               # (a crowded slot alone: no pair was lost on the way to it)
        else:
            assert printed == 0, (where, v)
    if row == "chunked":   # (the database went up in chunks)
        assert sum("chunk work queued" in ln for ln in seg) == 4, (where, seg[:8])
    else:
        assert not any("chunk work queued" in ln for ln in seg), where
    # 2. the answers
    assert got["wrong"] == [], (where, got["wrong"])
    if flags & PAIRWISE_ONLY and form == "device":
        assert got["nshared_compared"], where


@pytest.mark.parametrize("row,names", list(_groups()))
def test_capacity_edges_on_every_path(hip_lib, row, names):
    env_extra, jobs, _ = ROWS[row]
    out, lines = _run(names, jobs, env_extra)
    assert [res["name"] for res in out] == list(names)
    for name, res in zip(names, out):
        c = sc.case(name)
        assert res["H"] == c.H <= sc.MAX_H and res["n_refs"] == c.n_refs
        assert res["pairs"] > 0 and res["overlapping"] > 3 and res["hot_seen"]     # (the comparisons compare something)
        assert all(n >= 799 for n in res["hot_row_pairs"]) and sum(res["row_pairs"]) > 0   # (a hot hash's holder: a row of all its holders)
        for job in jobs:
            flags, form = job.split(":")
            _check_build(row, name, int(flags), form, res["builds"][job], lines)


def test_a_spilled_build_leaves_nothing_behind(hip_lib):
    """One process: a spilled case, its neighbour one pair below the capacity, the spilled case again -- full handle and train
    handle.  The second build reports no side list, the third reports and answers exactly what the first did (the marked-bucket
    bits, the counters and the side-list arrays all come from the library's buffer cache)."""
    a, b = sc.NEIGHBOURS
    names = [a, b, a]
    out, lines = _run(names, ["0:host", "8:host"], {})
    assert [res["name"] for res in out] == names
    for job in ("0:host", "8:host"):
        flags = int(job.split(":")[0])
        first, mid, third = (res["builds"][job] for res in out)
        for name, got in zip(names, (first, mid, third)):   # each against the model and the oracle: the third answers as the first
            _check_build("default", name, flags, "host", got, lines)
        assert mid["n_spilled_buckets"] == 0 == mid["n_spilled_pairs"]
        assert first["n_spilled_buckets"] == 1 and first["n_spilled_pairs"] == 4097
        assert {k: v for k, v in third.items() if k != "key"} == {k: v for k, v in first.items() if k != "key"}
