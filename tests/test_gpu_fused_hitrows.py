"""GPU: the fused run step (k_step_fused behind run_device_pipelined) whose 1024-lane lookups hand their hits to the reducer
of the next launch as HIT ROWS -- per (counter set, bin of 4096 references, lookup workgroup) a count word and up to 63 entries,
written with plain stores and never cleared -- instead of one atomic per (workgroup, reference) into the dense replica rows.
What does not fit a row goes to the dense rows and stamps the set's overflow word; only then does the reducer read them.

Every check compares the rows of run_device_pipelined bit for bit with the rows run_device gives for the same sample on a
handle of its own; one sample per scenario is also compared with the CPU oracle.  Databases and exact-size samples are those
of test_gpu_fused_roles / test_gpu_fused_replicas (300 and 4500 clustered references, clamp, isolate; 30 000, 262 144 and
524 288 hashes: the smallest samples that take the 256-lane geometry and the 1024-lane tiles of one and of two hashes), plus

    edges       4095, 4096, 4097 and 8193 references of six hashes; references 4092 .. 4099 are one cluster (its members
                straddle the edge between bin 0 and bin 1); the sample holds the last references of bin 0, the first of bin 1,
                the last ones of the database (the partial last bin, N mod 4 = 3, 0, 1, 1) and reference 0
    dense120    120 references of eight hashes, 60 of them in clusters of three; the sample holds all of them, so ONE tile
                finds 120 references of one bin, on shared hashes too: both count sets overflow a row of 63 entries
    spread      1 000 000 / 600 000 / 524 288 hashes: the clustered references of n4500 (or a few of them) among in-range
                hashes nobody holds, so that every tile of the sample has hits and every row of the step is non-empty

Each scenario runs in a child process (the debug switches are read once per process, behind YH_DEBUG_TUNING):

    edges       the four databases at both 1024-lane geometries, rows read two calls later and after a join
    overflow    dense120, n300 and n4500 at default capacity, then run_device, overlap and the stream lookup on the SAME handle
                (a dense counter left uncleared would be counted twice), and pipelined steps again
    small       the same with YH_HITROW_ENTS=2: rows of two entries, nearly every hit takes the overflow path
    isolate     one entry's count reaches the whole tile (2048: the width edge of an entry)
    clamp       140 000 references: more than 32 bins, the dense hand-over
    stale       hits, hits, fewer hits, fewer, none, none, hits, hits at 524 288 hashes (entries beyond a row's count are an
                earlier step's), then 1 000 000, 1 000 000, 600 000, 600 000, 1 000 000 (rows of workgroups beyond the
                second sample's tiles are the first sample's)
    geometry    30 000 <-> 524 288 <-> 262 144 hashes alternate: a hit-row step is reduced by a launch of another geometry
                and vice versa; rows after exactly two further calls, after a join following one call, and after a drain
    legacy      YH_NO_HITROWS=1: the dense hand-over gives the same rows

The capacity edges -- 32 | 33 bins, rows of 15 .. 64 entries, the allocation's growth, 2048 | 2049 tiles: test_gpu_fused_edges.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def edge_database(n):
    """n references of six distinct hashes below 2^40; 4092 .. 4099 (those that exist) hold the first three hashes of the first."""
    rng = np.random.default_rng(900 + n)
    pool = np.unique(rng.integers(1, 1 << 40, size=6 * n + 4096, dtype=np.uint64))[:6 * n]
    refs = [np.array(a) for a in rng.permutation(pool).reshape(n, 6)]
    cluster = np.array([j for j in range(4092, 4100) if j < n])
    for j in cluster[1:]:
        refs[j][:3] = refs[cluster[0]][:3]
    return [np.sort(a) for a in refs], cluster


def edge_samples(refs, cluster):
    import test_gpu_fused_roles as roles

    n = len(refs)
    ids = sorted({j for j in (0, 1, 2047, 4094, 4095, 4096, 4097, 4098, n - 3, n - 2, n - 1) if 0 <= j < n})
    top = int(max(a[-1] for a in refs))
    core = np.unique(np.concatenate([refs[j] for j in ids]))
    return {f"clusters@{s}": roles.exact(core, s, top) for s in (262_144, 524_288)}


def dense120():
    rng = np.random.default_rng(77)
    pool = np.unique(rng.integers(1, 1 << 40, size=120 * 8 + 512, dtype=np.uint64))[:120 * 8]
    refs = [np.array(a) for a in rng.permutation(pool).reshape(120, 8)]
    for c in range(20):     # clusters of three: members two and three hold four / six of the first member's hashes
        refs[3 * c + 1][:4] = refs[3 * c][:4]
        refs[3 * c + 2][:6] = refs[3 * c][:6]
    return [np.sort(a) for a in refs], np.arange(60)


def spread(core, size, held, seed):
    """`core` among in-range hashes nobody holds, evenly over the range: exactly `size` ascending distinct hashes."""
    rng = np.random.default_rng(seed)
    pad = np.setdiff1d(np.unique(rng.integers(0, int(held[-1]), size=size + size // 2, dtype=np.uint64)), held)
    pad = pad[np.linspace(0, pad.size - 1, size - core.size).astype(np.int64)]
    out = np.union1d(core, pad)
    assert out.size == size
    return out


class Bench:
    """One database: its samples on the device, the reference rows (run_device on a handle of its own), and the calls."""

    def __init__(self, name, refs, samples, check, oracle_label=None):
        import torch

        from oracle import oracle
        from yacht_amd import synth

        self.torch, self.name, self.check, self.smp = torch, name, check, samples
        self.values, self.offsets = synth.pack(refs)
        self.n = len(refs)
        self.d_s = {k: torch.from_numpy(s.view(np.int64).copy()).to("cuda") for k, s in samples.items()}
        with self.fresh() as h:
            self.want = {label: self.rows_plain(h, label) for label in samples}
        if oracle_label:
            s = samples[oracle_label]
            ov = oracle.overlap(self.values, self.offsets, s, threads=4)
            e, m = oracle.exclusive(self.values, self.offsets, ov > 0, s)
            check(np.array_equal(self.want[oracle_label], np.stack([ov, np.where(ov > 0, e, 0), np.where(ov > 0, m, 0)])),
                  f"{name} run_device of {oracle_label} differs from the oracle")

    def fresh(self):
        from yacht_amd import _lib
        from yacht_amd.engine import RefDB

        h = RefDB(self.values, self.offsets)
        h.set_lookup(_lib.YH_LOOKUP_INDEXED)
        return h

    def bufs(self, k=3):
        return [self.torch.empty((3, self.n), dtype=self.torch.int32, device="cuda") for _ in range(k)]

    def rows_plain(self, h, label):
        o = self.torch.full((3, self.n), -1, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        h.run_device(self.d_s[label].data_ptr(), self.smp[label].size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        h.synchronize()
        return o.cpu().numpy().view(np.uint32)

    def call(self, h, label, o):
        o.fill_(-1)
        self.torch.cuda.synchronize()        # (the fill runs on torch's stream, the step on the handle's)
        h.run_device_pipelined(self.d_s[label].data_ptr(), self.smp[label].size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())

    def same(self, o, label, what):
        got = o.cpu().numpy().view(np.uint32)
        for k, row in enumerate(("overlap", "n_excl", "n_match")):
            self.check(np.array_equal(got[k], self.want[label][k]), f"{self.name} {what}: {row} of {label} differs from run_device")

    def sequence(self, h, seq, what):
        """the calls of `seq` back to back: each one's rows exactly two calls later, the last two after the join"""
        bufs = self.bufs()
        for i, label in enumerate(seq):
            self.call(h, label, bufs[i % 3])
            if i == 0:
                self.torch.cuda.synchronize()
                self.check(bool((bufs[0][0] == -1).all()), f"{self.name} {what}: the first pipelined call wrote its rows at once (not the fused launch)")
            if i >= 2:
                self.torch.cuda.synchronize()
                self.same(bufs[(i - 2) % 3], seq[i - 2], f"{what}, call {i - 2} read two calls later")
        h.run_device_join()
        h.synchronize()
        self.same(bufs[(len(seq) - 1) % 3], seq[-1], f"{what}, last call after the join")
        if len(seq) > 1:
            self.same(bufs[(len(seq) - 2) % 3], seq[-2], f"{what}, last call but one after the join")

    def joins(self, h, labels, what):
        """a join after one call, and after two calls (a drain with a reducer AND an exclusive pass pending)"""
        bufs = self.bufs(2)
        for a in labels:
            self.call(h, a, bufs[0])
            h.run_device_join()
            h.synchronize()
            self.same(bufs[0], a, f"{what}, join after one call")
            for b in labels:
                self.call(h, a, bufs[0])
                self.call(h, b, bufs[1])
                h.run_device_join()
                h.synchronize()
                self.same(bufs[0], a, f"{what}, join after two calls ({a}, {b}), first")
                self.same(bufs[1], b, f"{what}, join after two calls ({a}, {b}), second")

    def at_rest(self, h, label, what):
        """every other entry point that shares the dense counters, on the SAME handle"""
        from yacht_amd import _lib

        want = self.want[label]
        self.check(np.array_equal(self.rows_plain(h, label), want), f"{self.name} at rest, {what}: run_device differs")
        self.check(np.array_equal(h.overlap(self.smp[label]), want[0]), f"{self.name} at rest, {what}: overlap differs")
        h.set_lookup(_lib.YH_LOOKUP_STREAM)
        self.check(np.array_equal(h.overlap(self.smp[label]), want[0]), f"{self.name} at rest, {what}: overlap (stream lookup) differs")
        self.check(np.array_equal(self.rows_plain(h, label), want), f"{self.name} at rest, {what}: run_device (stream lookup) differs")
        h.set_lookup(_lib.YH_LOOKUP_INDEXED)


def _base(names):
    import test_gpu_fused_roles as roles

    dbs = roles.databases()
    return {k: (dbs[k][0], roles.samples_of(*dbs[k])) for k in names}


def sc_edges(check, info):
    for n in (4095, 4096, 4097, 8193):
        refs, cluster = edge_database(n)
        b = Bench(f"edge{n}", refs, edge_samples(refs, cluster), check, oracle_label="clusters@524288")
        hit = int((b.want["clusters@524288"][0] > 0).sum())
        info[f"edge{n}"] = hit
        last = min(n - 1, 4099)
        check(all(b.want["clusters@524288"][0][j] > 0 for j in (min(4095, n - 1), last, n - 1)), f"edge{n}: the edge references are not hit")
        with b.fresh() as h:
            b.sequence(h, ["clusters@524288", "clusters@262144", "clusters@524288", "clusters@524288", "clusters@262144", "clusters@262144"], "edges")
            b.at_rest(h, "clusters@524288", "behind the pipelined steps")


def sc_overflow(check, info, names=("dense120", "n300", "n4500")):
    import test_gpu_fused_roles as roles

    todo = _base([k for k in names if k != "dense120"])
    if "dense120" in names:
        refs, clustered = dense120()
        todo["dense120"] = (refs, roles.samples_of(refs, clustered))
    for name, (refs, smp) in todo.items():
        smp = {k: v for k, v in smp.items() if k.split("@")[1] != "30000" and k.split("@")[0] in ("all", "clusters", "miss")}
        b = Bench(name, refs, smp, check, oracle_label="all@524288")
        info[name] = int((b.want["all@524288"][0] > 0).sum())
        with b.fresh() as h:
            b.sequence(h, ["all@524288", "clusters@262144", "miss@524288", "all@262144", "all@524288", "clusters@524288"], "overflow")
            b.at_rest(h, "all@524288", "behind the pipelined steps")
            b.sequence(h, ["clusters@524288", "all@524288", "all@524288"], "overflow again")
            b.at_rest(h, "clusters@524288", "behind both")


def sc_small(check, info):
    sc_overflow(check, info, names=("n300", "n4500"))


def sc_isolate(check, info):
    import test_gpu_fused_replicas as reps

    refs, clustered = reps._databases()["isolate"]
    import test_gpu_fused_roles as roles

    smp = reps._samples("isolate", refs, clustered)
    # ... and the first big reference alone in front of hashes nobody holds: the first two tiles are 2048 hashes of it each
    smp["whole0@524288"] = roles.exact(refs[0], 524_288, int(max(a[-1] for a in refs)))
    b = Bench("isolate", refs, smp, check, oracle_label="clusters@524288")
    info["isolate"] = int(b.want["clusters@524288"][0].max())
    check(int(b.want["whole0@524288"][0][0]) == 4096, "isolate: the first reference is not whole in its own sample")
    with b.fresh() as h:
        b.sequence(h, ["clusters@524288", "whole0@524288", "miss@524288", "whole0@524288", "clusters@524288"], "isolate")
        b.at_rest(h, "clusters@524288", "behind the pipelined steps")


def sc_clamp(check, info):
    import test_gpu_fused_replicas as reps

    refs, clustered = reps._databases()["clamp"]
    smp = {k: v for k, v in reps._samples("clamp", refs, clustered).items() if k in ("clusters@524288", "miss@524288", "clusters@262144")}
    b = Bench("clamp", refs, smp, check, oracle_label="clusters@524288")
    info["clamp"] = b.n
    with b.fresh() as h:
        b.sequence(h, ["clusters@524288", "clusters@262144", "miss@524288", "clusters@524288"], "clamp")
        b.at_rest(h, "clusters@524288", "behind the pipelined steps")


def sc_stale(check, info):
    import test_gpu_fused_roles as roles

    refs, clustered = roles.databases()["n4500"]
    held = np.unique(np.concatenate(refs))
    many = np.unique(np.concatenate([refs[j] for j in clustered]))
    few = np.unique(np.concatenate([refs[j] for j in clustered[:40]]))
    smp = {"many@524288": spread(many, 524_288, held, 1), "few@524288": spread(few, 524_288, held, 2),
           "none@524288": spread(many[:0], 524_288, held, 3), "many@1000000": spread(many, 1_000_000, held, 4),
           "few@600000": spread(few, 600_000, held, 5)}
    b = Bench("n4500", refs, smp, check, oracle_label="many@524288")
    info["stale"] = {k: int((v[0] > 0).sum()) for k, v in b.want.items()}
    tiles = smp["many@1000000"].reshape(-1, 2000)     # (every stretch of the sample holds hits: the rows of all its tiles are non-empty)
    check(all(np.isin(t, many).any() for t in tiles), "stale: a stretch of the 1 000 000-hash sample without a hit")
    with b.fresh() as h:
        b.sequence(h, ["many@524288", "many@524288", "few@524288", "few@524288", "none@524288", "none@524288", "many@524288", "many@524288"], "stale entries")
        b.sequence(h, ["many@1000000", "many@1000000", "few@600000", "few@600000", "many@1000000"], "stale rows")
        b.at_rest(h, "many@524288", "behind the pipelined steps")


def sc_geometry(check, info, names=("n300", "n4500")):
    from yacht_amd import _lib

    for name, (refs, smp) in _base(names).items():
        smp = {k: v for k, v in smp.items() if k.split("@")[0] in ("clusters", "miss")}
        b = Bench(name, refs, smp, check, oracle_label="clusters@262144")
        info[name] = int((b.want["clusters@524288"][0] > 0).sum())
        order = [30_000, 524_288, 262_144, 524_288, 30_000, 262_144, 30_000]
        seq = [f"{'clusters' if i % 3 != 2 else 'miss'}@{s}" for i, s in enumerate(order + order)]
        with b.fresh() as h:
            check(h.lookup_choice(524_288) == _lib.YH_LOOKUP_INDEXED, f"{name}: the indexed lookup was not chosen")
            b.sequence(h, seq, "geometry")
            b.joins(h, [f"clusters@{s}" for s in (30_000, 262_144, 524_288)], "geometry")
            b.at_rest(h, "clusters@524288", "behind the pipelined steps")


def sc_legacy(check, info):
    sc_geometry(check, info, names=("n4500",))
    sc_overflow(check, info, names=("n300",))


SCENARIOS = {
    # name: (function, environment, checks at least)
    "edges": (sc_edges, {}, 100),
    "overflow": (sc_overflow, {}, 100),
    "small": (sc_small, {"YH_DEBUG_TUNING": "1", "YH_HITROW_ENTS": "2"}, 60),
    "isolate": (sc_isolate, {}, 15),
    "clamp": (sc_clamp, {}, 15),
    "stale": (sc_stale, {}, 40),
    "geometry": (sc_geometry, {}, 150),
    "legacy": (sc_legacy, {"YH_DEBUG_TUNING": "1", "YH_NO_HITROWS": "1"}, 100),
}


def _collect(which):
    failures, n_checks, info = [], [0], {}

    def check(ok, what):
        n_checks[0] += 1
        if not ok and len(failures) < 20:
            failures.append(what)

    SCENARIOS[which][0](check, info)
    return failures, n_checks[0], info


WORKER = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_fused_hitrows as t
failures, n_checks, info = t._collect(sys.argv[2])
print(json.dumps({"failures": failures, "checks": n_checks, "info": info}))
"""


@pytest.mark.parametrize("which", list(SCENARIOS))
def test_fused_hitrows(hip_lib, which):
    env = {k: v for k, v in os.environ.items() if not k.startswith("YH_")}
    env.update(SCENARIOS[which][1])
    r = subprocess.run([sys.executable, "-c", WORKER, ROOT, which], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out["checks"], out["info"])
    assert out["checks"] >= SCENARIOS[which][2]
    if which == "isolate":
        assert out["info"]["isolate"] >= 4096      # (both big references whole; a tile's entry for one of them counts up to 2048)
    if which == "clamp":
        assert out["info"]["clamp"] == 140_000
    assert not out["failures"], "\n".join(out["failures"])
