"""GPU: the hit rows of the fused run step (k_step_fused behind run_device_pipelined) where tests/test_gpu_fused_hitrows.py does
not go: bins 3 .. 31 and the limit of 32 bins from both sides, rows of exactly 15, 16, 31, 32, 47, 48, 63 and 64 entries (the
sector edges of the reducer's reads and the first claim that overflows), hit tables with three and more references on one
home slot, the growth of the row allocation with steps pending, and the cap of 2048 tiles between two 1024-lane steps.

The databases, samples and call sequences are those of tests/fused_cases.py; that each reaches the state it is named for is
proved on the CPU by tests/test_fused_cases_cpu.py.  Every check is exact (np.array_equal): the three rows of every pipelined
step against run_device on a handle of its own (Bench of test_gpu_fused_hitrows), one sample per scenario against
oracle.overlap / oracle.exclusive, and run_device, overlap and the stream lookup on the SAME handle behind the steps (a
dense counter an overflow left uncleared counts twice there).

Exact counts cannot tell a step that went dense from one that left rows.  So every child runs with YH_TRACE_HITROWS=1 (behind
YH_DEBUG_TUNING), and the line every fused step prints from the handle's host state -- tiles, rows or dense, capacity, whether
the allocation grew and how many draining launches that took -- must equal, line for line, what the mirror of
tests/fused_cases.py predicts for the calls made; the paths and capacities the scenarios are named for are also written
out below.  A step that silently took another path fails.

One child process per scenario (the switches are read once per process); after a child that did not come back or died on a
signal nothing more is started on the GPU.

    bins32      131 072 references: quarters (ONE tile hits a reference in every 1024-reference quarter of all 32 bins) and corners
                (first and last references of bins 0 .. 3, 15, 16, 30, 31, clusters across bin edges, spread over many tiles) at both
                1024-lane geometries, alternating with 30 000-hash samples: a 256-lane reducer sums every (bin, quarter)
    bins33      131 073 references, the same sequence: every step takes the dense hand-over
    fill        every k in 15 .. 64 with a different k before, behind, and two calls earlier in the same counter set
    crowded     the same shape with three and more hit references on one home slot
    growth      524 288, 1 048 576, 1 048 577, 1 048 577, 4 194 304, 524 288, 4 194 304 hashes on one handle: capacity 512, 512, 768,
                768, 2048, 2048, 2048, each growth draining two pending steps; then a handle whose first allocation happens with two
                256-lane steps pending
    tilecap     4 194 304 (2048 tiles, rows), 4 194 305 (2049, dense), twice, then 1 048 577

Measured on an MI355X, the scenario's own work (and the whole child, with the start of Python and the runtime): bins32 1.9 s
(2.5 s), bins33 1.7 s (2.4 s), fill 1.6 s (2.3 s), crowded 1.6 s (2.3 s), growth 1.9 s (2.5 s), tilecap 1.9 s (2.5 s): 14.9 s for
the file.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import fused_cases as fc
from test_gpu_fused_hitrows import Bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_child_lost = []        # set by the first child that did not come back or died on a signal: nothing more is started on the GPU


class EdgeBench(Bench):
    """Bench that also keeps the log the mirror predicts the trace lines from: handles opened, pipelined calls, joins."""

    def __init__(self, *args, **kwargs):
        self.log = []
        super().__init__(*args, **kwargs)

    def fresh(self):
        self.log.append(("handle", self.n))
        return super().fresh()

    def call(self, h, label, o):
        self.log.append(("step", int(self.smp[label].size)))
        super().call(h, label, o)

    def sequence(self, h, seq, what):
        print(f"[fused edges] {self.name}: {what}, {len(seq)} calls", file=sys.stderr, flush=True)
        super().sequence(h, list(seq), what)
        self.log.append(("join",))


def _whole(b, check, label, ids, what):
    check(bool((b.want[label][0][np.asarray(ids)] == fc.PER_REF).all()), f"{b.name}: {what} are not whole in {label}")


def sc_bins(check, info, n):
    db = fc.bins_database(n)
    b = EdgeBench(db.name, db.refs, fc.bins_samples(db), check, oracle_label="corners@524288")
    corners, quarters = fc.bins_ids(db)
    for size in (262_144, 524_288, 30_000):
        _whole(b, check, f"quarters@{size}", quarters, "the references of the quarters")
        _whole(b, check, f"corners@{size}", corners, "the corner references")
    info["hit"] = int((b.want["quarters@524288"][0] > 0).sum())
    with b.fresh() as h:
        b.sequence(h, fc.BINS_SEQ, "bins")
        b.at_rest(h, "quarters@524288", "behind the pipelined steps")
        b.sequence(h, ("corners@262144", "quarters@30000", "quarters@524288"), "bins again")
    return b.log


def sc_bins32(check, info):
    return sc_bins(check, info, 131_072)


def sc_bins33(check, info):
    return sc_bins(check, info, 131_073)


def sc_fill(check, info):
    db = fc.fill_database()
    b = EdgeBench("fill", db.refs, fc.fill_samples(db), check, oracle_label="pairs63@524288")
    _whole(b, check, "single64@524288", db.singles, "the 64 single references")
    info["hit"] = int((b.want["pairs64@524288"][0] > 0).sum())
    with b.fresh() as h:
        b.sequence(h, fc.FILL_SEQ[:21], "fill")
        b.at_rest(h, "single64@524288", "behind a row of 64 claims")
        b.sequence(h, fc.FILL_SEQ[21:], "fill, both geometries")
        b.at_rest(h, "pairs64@524288", "behind a row of 64 claims, half of them second-set entries")
    return b.log


def sc_crowded(check, info):
    db = fc.crowded_database()
    b = EdgeBench("crowded", db.refs, fc.crowded_samples(db), check, oracle_label="crowd_full@524288")
    _whole(b, check, "crowd8@524288", db.crowd, "the crowd's references")
    info["hit"] = int((b.want["crowd_full@524288"][0] > 0).sum())
    with b.fresh() as h:
        b.sequence(h, fc.CROWDED_SEQ, "crowded")
        b.at_rest(h, "crowd_full@524288", "behind rows filled by single hits")
    return b.log


SECOND_HANDLE = ("small@30000", "small@30000", "spread@524288", "spread@1048577", "small@30000")


def sc_growth(check, info):
    db = fc.fill_database()
    smp = {k: v for k, v in fc.growth_samples().items() if k != "spread@4194305"}
    b = EdgeBench("fill", db.refs, smp, check, oracle_label="spread@1048577")
    info["hit"] = int((b.want["spread@4194304"][0] > 0).sum())
    with b.fresh() as h:
        b.sequence(h, [f"spread@{s}" for s in fc.GROWTH_SEQ], "growth")
        b.at_rest(h, "spread@1048577", "behind the grown allocation")
    with b.fresh() as h:
        b.sequence(h, SECOND_HANDLE, "first allocation with steps pending")
    return b.log


def sc_tilecap(check, info):
    db = fc.fill_database()
    smp = {k: v for k, v in fc.growth_samples().items() if k in ("spread@4194304", "spread@4194305", "spread@1048577")}
    b = EdgeBench("fill", db.refs, smp, check, oracle_label="spread@4194305")
    info["hit"] = int((b.want["spread@4194305"][0] > 0).sum())
    with b.fresh() as h:
        b.sequence(h, [f"spread@{s}" for s in fc.TILECAP_SEQ], "tile cap")
        b.at_rest(h, "spread@4194304", "behind the pipelined steps")
    return b.log


SCENARIOS = {
    # name: (function, checks at least)
    "bins32": (sc_bins32, 50),
    "bins33": (sc_bins33, 50),
    "fill": (sc_fill, 90),
    "crowded": (sc_crowded, 40),
    "growth": (sc_growth, 40),
    "tilecap": (sc_tilecap, 20),
}


def worker(which):
    t0 = time.perf_counter()
    failures, n_checks, info = [], [0], {}

    def check(ok, what):
        n_checks[0] += 1
        if not ok and len(failures) < 20:
            failures.append(what)

    log = SCENARIOS[which][0](check, info)
    print(json.dumps({"failures": failures, "checks": n_checks[0], "info": info, "expected": fc.predict(log),
                      "seconds": round(time.perf_counter() - t0, 2)}))


WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_fused_edges as t
t.worker(sys.argv[2])
"""


def _named_for(which, got):
    """the path, capacity and growth each scenario is named for, written out (not taken from the mirror)"""
    steps = [(ln["tiles"], ln["path"], ln["capacity"], ln["grew"], ln["drained"]) for ln in got]
    if which in ("bins32", "bins33"):
        assert all(ln["refs"] == (131_072 if which == "bins32" else 131_073) for ln in got)      # 32 bins of 4096, and one reference more
        for ln in got:
            rows = which == "bins32" and ln["lanes"] == 1024
            assert ln["path"] == ("rows" if rows else "dense"), ln
            assert ln["capacity"] == (512 if which == "bins32" else 0), ln
        assert {ln["lanes"] for ln in got} == {256, 1024} and {ln["tiles"] for ln in got if ln["lanes"] == 1024} == {256}
    elif which in ("fill", "crowded"):
        assert all(s == (256, "rows", 512, int(i == 0), 0) for i, s in enumerate(steps)), steps
    elif which == "growth":
        assert steps[:7] == [(256, "rows", 512, 1, 0), (512, "rows", 512, 0, 0), (513, "rows", 768, 1, 2), (513, "rows", 768, 0, 0),
                             (2048, "rows", 2048, 1, 2), (256, "rows", 2048, 0, 0), (2048, "rows", 2048, 0, 0)], steps
        assert steps[7:] == [(118, "dense", 0, 0, 0), (118, "dense", 0, 0, 0), (256, "rows", 512, 1, 0), (513, "rows", 768, 1, 2),
                             (118, "dense", 768, 0, 0)], steps
    elif which == "tilecap":
        assert steps == [(2048, "rows", 2048, 1, 0), (2049, "dense", 2048, 0, 0), (2048, "rows", 2048, 0, 0), (2049, "dense", 2048, 0, 0),
                         (513, "rows", 2048, 0, 0)], steps
        assert all(ln["lanes"] == 1024 for ln in got)


@pytest.mark.parametrize("which", list(SCENARIOS))
def test_fused_edges(hip_lib, which):
    assert not _child_lost, f"not started: the worker of {_child_lost[0]} did not come back or died on a signal"
    env = {k: v for k, v in os.environ.items() if not k.startswith("YH_")}
    env.update({"YH_DEBUG_TUNING": "1", "YH_TRACE_HITROWS": "1"})
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-c", WORKER, ROOT, which], capture_output=True, text=True, env=env, timeout=240)
    except subprocess.TimeoutExpired as e:
        _child_lost.append(which)
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("the worker did not come back; it was at:\n" + "\n".join(ln for ln in err.splitlines() if ln.startswith("[fused edges]"))[-600:])
    if r.returncode < 0 or (r.returncode != 0 and "illegal memory access" in r.stderr):
        _child_lost.append(which)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[fused edges] {which}: {out['checks']} checks, worker {out['seconds']} s, child {time.perf_counter() - t0:.2f} s, {out['info']}")
    assert out["checks"] >= SCENARIOS[which][1]
    assert not out["failures"], "\n".join(out["failures"])
    # the path every step took: the launches of the lookups, in call order, against the mirror and against the scenario's name
    got = [ln for ln in r.stderr.splitlines() if ln.startswith("[yh hitrows] ")]
    assert got == out["expected"], "\n".join(["traced:"] + got + ["predicted:"] + out["expected"])
    _named_for(which, [fc.parse(ln) for ln in got])
