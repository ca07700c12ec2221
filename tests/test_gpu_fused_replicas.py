"""GPU: the fused run step (k_step_fused behind run_device_pipelined) with its hit counters spread over 1 .. 16 replica rows,
the row count carried from a step's lookup to its reducer in the next launch, and the counters zero at rest for every path
that shares them with fewer rows.

Every check compares the rows of run_device_pipelined bit for bit with the rows run_device gives for the same sample on a
handle of its own; one sample per launch geometry and database is also compared with the CPU oracle.  Databases and
exact-size samples are those of test_gpu_fused_roles (300 and 4500 clustered references; 30 000, 262 144 and 524 288
hashes: the smallest samples that take the 256-lane geometry and the 1024-lane tiles of one and of two hashes per lane), plus

    ragged      the 300-reference database without its last one, two and three references (N = 3, 2, 1 mod 4)
    clamp       140 000 references of four hashes, 60 of them in clusters: 8 replica rows fit the counters' allocation
                (rows x references <= 2^21), whatever count is asked for
    isolate     two references of 4096 hashes that share half of them, beside 250 small ones; the sample holds both whole
                and is padded to 524 288 hashes with in-range hashes nobody holds, so each of its 256 tiles finds hashes of
                both and every workgroup flushes the same counters

The scenarios run in child processes (the switch is read once per process, behind YH_DEBUG_TUNING): YH_FUSED_REPS = 1, unset
(each geometry's own default) and 16.

    follows     consecutive calls alternate 30 000 <-> 524 288 <-> 262 144 hashes, so a step's lookup and its reducer run in
                launches of different geometry (and, by default, different row counts); rows read after exactly two further
                calls without a join, and after a join following one call and following two
    at rest     pipelined steps at the largest geometry, a join, then run_device, overlap and the stream lookup on the SAME
                handle give the reference rows (a row left uncleared would be counted twice); and the reverse order
    fused       after one pipelined call (no join) its overlap row still holds the 0xFFFFFFFF put there
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


def _databases():
    """name -> (refs, clustered ids)"""
    import test_gpu_fused_roles as roles
    from yacht_amd import synth

    base = roles.databases()
    out = dict(base)
    refs, clustered = base["n300"]
    for drop in (1, 2, 3):
        out[f"n{300 - drop}"] = (refs[:300 - drop], clustered[clustered < 300 - drop])
    # clamp: 140 000 x 4 distinct hashes below 2^40, cut from one ascending draw; the first 60 references are 20 clusters of
    # three (members two and three hold the first member's first two / three hashes instead of their own)
    rng = np.random.default_rng(73)
    n = 140_000
    pool = np.unique(rng.integers(1, 1 << 40, size=4 * n + 4096, dtype=np.uint64))[:4 * n]
    tiny = [np.array(a) for a in rng.permutation(pool).reshape(n, 4)]
    for c in range(20):
        tiny[3 * c + 1][:2] = tiny[3 * c][:2]
        tiny[3 * c + 2][:3] = tiny[3 * c][:3]
    out["clamp"] = ([np.sort(a) for a in tiny], np.arange(60))
    # isolate
    rng = np.random.default_rng(74)
    big = synth.clustered_refs(rng, 1, (1.0, 0.5), 4096, scaled=roles.SCALED)
    out["isolate"] = (big + synth.independent_refs(rng, 250, 80, 0.3, 40, 160, scaled=roles.SCALED), np.arange(2))
    return out


def _samples(name, refs, clustered):
    """label -> sample, labels as in test_gpu_fused_roles.samples_of"""
    import test_gpu_fused_roles as roles

    if name == "isolate":
        held = np.unique(np.concatenate(refs))
        core = np.unique(np.concatenate([refs[0], refs[1]]))
        rng = np.random.default_rng(6)
        pad = np.setdiff1d(np.unique(rng.integers(0, int(held[-1]), size=700_000, dtype=np.uint64)), held)
        pad = pad[np.linspace(0, pad.size - 1, 524_288 - core.size).astype(np.int64)]     # (evenly over the range, distinct)
        both = np.union1d(core, pad)
        assert both.size == 524_288
        tiles = both.reshape(256, 2048)
        assert all(np.isin(t, refs[0]).any() and np.isin(t, refs[1]).any() for t in tiles), "a tile without hashes of both"
        miss = roles.exact(np.setdiff1d(pad[:20_000], held), 524_288, int(held[-1]))
        return {"clusters@524288": both, "miss@524288": miss}
    return roles.samples_of(refs, clustered)


def scenarios(check, info):
    import torch

    import test_gpu_fused_roles as roles
    from oracle import oracle
    from yacht_amd import _lib, synth
    from yacht_amd.engine import RefDB

    dev = "cuda"
    for name, (refs, clustered) in _databases().items():
        values, offsets = synth.pack(refs)
        n = len(refs)
        smp = _samples(name, refs, clustered)
        sizes = [s for s in roles.SIZES if f"clusters@{s}" in smp]
        d_s = {k: torch.from_numpy(s.view(np.int64).copy()).to(dev) for k, s in smp.items()}

        def rows_plain(h, label):
            o = torch.full((3, n), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            h.run_device(d_s[label].data_ptr(), smp[label].size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
            h.synchronize()
            return o.cpu().numpy().view(np.uint32)

        def call(h, label, o):
            o.fill_(-1)
            torch.cuda.synchronize()        # (the fill runs on torch's stream, the step on the handle's)
            h.run_device_pipelined(d_s[label].data_ptr(), smp[label].size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())

        def same(o, label, what):
            got = o.cpu().numpy().view(np.uint32)
            for k, row in enumerate(("overlap", "n_excl", "n_match")):
                check(np.array_equal(got[k], want[label][k]), f"{name} {what}: {row} of {label} differs from run_device")

        def fresh():
            h = RefDB(values, offsets)
            h.set_lookup(_lib.YH_LOOKUP_INDEXED)
            return h

        # the reference rows, once: run_device on a handle of its own; one sample per geometry against the CPU oracle
        with fresh() as h:
            want = {label: rows_plain(h, label) for label in smp}
        for size in sizes:
            label = f"clusters@{size}"
            ov = oracle.overlap(values, offsets, smp[label], threads=4)
            e, m = oracle.exclusive(values, offsets, ov > 0, smp[label])
            check(np.array_equal(want[label], np.stack([ov, np.where(ov > 0, e, 0), np.where(ov > 0, m, 0)])),
                  f"{name} run_device of {label} differs from the oracle")
            check(int((want[label][0] > 0).sum()) >= clustered.size, f"{name} {label}: the clustered references are not all hit")
        top = sizes[-1]
        hi, lo = f"clusters@{top}", f"miss@{top}"
        info[name] = {"n": n, "hit": int((want[hi][0] > 0).sum())}

        # follows: the geometry, and with it the row count, changes from launch to launch
        order = [s for s in (30_000, 524_288, 262_144, 524_288, 30_000, 262_144, 30_000) if s in sizes]
        seq = [f"{'clusters' if i % 3 != 2 else 'miss'}@{s}" for i, s in enumerate(order + order)]
        with fresh() as h:
            check(h.lookup_choice(top) == _lib.YH_LOOKUP_INDEXED, f"{name}: the indexed lookup was not chosen")
            bufs = [torch.empty((3, n), dtype=torch.int32, device=dev) for _ in range(3)]
            for i, label in enumerate(seq):
                call(h, label, bufs[i % 3])
                if i == 0:      # the launch is the fused one: this call's rows come with the calls behind it
                    torch.cuda.synchronize()
                    check(bool((bufs[0][0] == -1).all()), f"{name}: the first pipelined call wrote its rows at once (not the fused launch)")
                if i >= 2:      # complete after exactly two further calls
                    torch.cuda.synchronize()
                    same(bufs[(i - 2) % 3], seq[i - 2], f"follows, call {i - 2} read two calls later")
            h.run_device_join()
            h.synchronize()
            same(bufs[(len(seq) - 1) % 3], seq[-1], "follows, last call after the join")
            same(bufs[(len(seq) - 2) % 3], seq[-2], "follows, last call but one after the join")
            for a in sizes:     # a join after one call, and after two calls of different geometry
                call(h, f"clusters@{a}", bufs[0])
                h.run_device_join()
                h.synchronize()
                same(bufs[0], f"clusters@{a}", "join after one call")
                for b in sizes:
                    call(h, f"clusters@{a}", bufs[0])
                    call(h, f"clusters@{b}", bufs[1])
                    h.run_device_join()
                    h.synchronize()
                    same(bufs[0], f"clusters@{a}", f"join after two calls ({a}, {b}), first")
                    same(bufs[1], f"clusters@{b}", f"join after two calls ({a}, {b}), second")

        # at rest: every path that shares the counters, with fewer rows, behind and in front of the pipelined steps
        def others(h, what):
            got = rows_plain(h, hi)
            check(np.array_equal(got, want[hi]), f"{name} at rest, {what}: run_device differs")
            check(np.array_equal(h.overlap(smp[hi]), want[hi][0]), f"{name} at rest, {what}: overlap differs")
            h.set_lookup(_lib.YH_LOOKUP_STREAM)
            check(np.array_equal(h.overlap(smp[hi]), want[hi][0]), f"{name} at rest, {what}: overlap (stream lookup) differs")
            got = rows_plain(h, hi)
            check(np.array_equal(got, want[hi]), f"{name} at rest, {what}: run_device (stream lookup) differs")
            h.set_lookup(_lib.YH_LOOKUP_INDEXED)

        def pipelined(h, what):
            bufs = [torch.empty((3, n), dtype=torch.int32, device=dev) for _ in range(3)]
            for i, label in enumerate((hi, hi, lo, hi)):
                call(h, label, bufs[i % 3])
            h.run_device_join()
            h.synchronize()
            same(bufs[0], hi, f"at rest, {what}: last pipelined step")
            same(bufs[2], lo, f"at rest, {what}: pipelined step that hits nothing")

        with fresh() as h:
            pipelined(h, "pipelined first")
            others(h, "behind the pipelined steps")
            pipelined(h, "pipelined again")
        with fresh() as h:
            others(h, "on a fresh handle")
            pipelined(h, "behind the other paths")
            others(h, "behind both")


def _collect():
    failures, n_checks, info = [], [0], {}

    def check(ok, what):
        n_checks[0] += 1
        if not ok and len(failures) < 20:
            failures.append(what)

    scenarios(check, info)
    return failures, n_checks[0], info


WORKER = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_fused_replicas as t
failures, n_checks, info = t._collect()
print(json.dumps({"failures": failures, "checks": n_checks, "info": info}))
"""


@pytest.mark.parametrize("reps", ["1", None, "16"], ids=["one", "default", "sixteen"])
def test_fused_replicas(hip_lib, reps):
    env = {k: v for k, v in os.environ.items() if not k.startswith("YH_")}
    if reps is not None:
        env.update({"YH_DEBUG_TUNING": "1", "YH_FUSED_REPS": reps})
    r = subprocess.run([sys.executable, "-c", WORKER, ROOT], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out["checks"], out["info"])
    assert out["checks"] > 300
    assert set(out["info"]) == {"n300", "n4500", "n299", "n298", "n297", "clamp", "isolate"}
    assert out["info"]["isolate"]["hit"] >= 2 and out["info"]["clamp"]["n"] == 140_000
    assert not out["failures"], "\n".join(out["failures"])
