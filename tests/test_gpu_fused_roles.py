"""GPU: the three roles of the fused run step (k_step_fused behind run_device_pipelined), the reducer's grouped reads at ragged
block ranges and the exclusive role at any size.

Every check compares the rows of run_device_pipelined bit for bit with the rows run_device gives for the same sample on a
handle of the same database; one sample per launch geometry is also compared with the CPU oracle.  Two small clustered
databases (helpers of yacht_amd.synth): 300 references (one reducer block, ragged) and 4500 (not a multiple of 4096: the
1024-lane reducer's second block is ragged; the 256-lane one's fifth).  Samples of 30 000, 262 144 and 524 288 hashes -- the
smallest that take the 256-lane geometry and the 1024-lane tiles of one and of two hashes per lane -- padded to their exact
size with hashes above everything the database holds.

    swings      work lists 0 -> maximal -> 0 -> ... from the first call of a fresh handle (a sample that hits nothing, then one
                holding every reference, or every clustered one where that does not fit the size); rows read after exactly two
                further calls, without a join
    capacity    the sample holding every reference: the work list at its capacity
    on time     join after one call and after two; set_stream and a run_device call in the middle of a pipeline
    rotation    two and three output buffers

The same scenarios run once more in a child process with YH_FUSED_EXCL_WGS=1 (read once per process, behind YH_DEBUG_TUNING):
the exclusive role as ONE workgroup, which walks every list by itself, the ones at capacity included.  That the launches are
the fused ones is checked by what a pipelined call leaves unwritten: after one call (no join) its overlap row still holds
the 0xFFFFFFFF put there.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# hashes below 2^40: with so few distinct hashes the directory takes its compact form (a bucket spans less than 2^32 hash values)
# only over a narrow range, and without the compact form the pipelined step is not the fused launch
SCALED = 1 << 24
SIZES = (30_000, 262_144, 524_288)      # 256 lanes | 1024 lanes x 1 hash | 1024 lanes x 2 hashes (yh_tile_shape_for)


def databases():
    """name -> (refs, clustered ids): 300 references of ~80 hashes, 200 of them in clusters of five; 4500 of ~40, 500 clustered."""
    from yacht_amd import synth

    out = {}
    for name, n_clusters, n_single, size, seed in (("n300", 40, 100, 80, 71), ("n4500", 100, 4000, 40, 72)):
        rng = np.random.default_rng(seed)
        refs = synth.clustered_refs(rng, n_clusters, (1.0, 0.9, 0.5, 0.25, 0.1), size, scaled=SCALED)
        refs += synth.independent_refs(rng, n_single, size, 0.3, size // 2, 2 * size, scaled=SCALED)
        order = rng.permutation(len(refs))      # clusters spread over the reducer's blocks
        refs = [refs[i] for i in order]
        clustered = np.flatnonzero(order < 5 * n_clusters)
        out[name] = (refs, clustered)
    return out


def exact(core, size, top):
    """`core` (ascending, distinct) widened to exactly `size` hashes by hashes above `top`, which nobody holds."""
    assert core.size <= size
    pad = np.uint64(top) + np.arange(1, size - core.size + 1, dtype=np.uint64) * np.uint64(977)
    return np.concatenate([core, pad])


def samples_of(refs, clustered):
    """label -> sample.  miss: in-range hashes no reference holds; clusters: every clustered reference whole; all: every
    reference whole (the work list at capacity); few: three clustered references and two others at half coverage."""
    rng = np.random.default_rng(5)
    held = np.unique(np.concatenate(refs))
    top = int(held[-1])
    miss = np.setdiff1d(np.unique(rng.integers(0, top, size=20_000, dtype=np.uint64)), held)
    cores = {"miss": miss, "clusters": np.unique(np.concatenate([refs[j] for j in clustered])), "all": held}
    other = np.setdiff1d(np.arange(len(refs)), clustered)
    few = [refs[j] for j in clustered[:3]] + [refs[j][::2] for j in other[:2]]
    cores["few"] = np.unique(np.concatenate(few))
    out = {}
    for size in SIZES:
        for label, core in cores.items():
            if core.size <= size:
                out[f"{label}@{size}"] = exact(core, size, top)
    return out


def scenarios(check):
    """Everything on this process's GPU; check(ok, what) collects."""
    import torch

    from oracle import oracle
    from yacht_amd import _lib, synth
    from yacht_amd.engine import RefDB

    dev = "cuda"
    for name, (refs, clustered) in databases().items():
        values, offsets = synth.pack(refs)
        n = len(refs)
        smp = samples_of(refs, clustered)
        d_s = {k: torch.from_numpy(s.view(np.int64).copy()).to(dev) for k, s in smp.items()}

        def rows_plain(h, label):
            o = torch.full((3, n), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            h.run_device(d_s[label].data_ptr(), smp[label].size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
            h.synchronize()
            return o.cpu().numpy().view(np.uint32)

        def call(h, label, o, fill=True):
            if fill:
                o.fill_(-1)
                torch.cuda.synchronize()        # (the fill runs on torch's stream, the step on the handle's)
            h.run_device_pipelined(d_s[label].data_ptr(), smp[label].size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())

        def same(o, label, what):
            got = o.cpu().numpy().view(np.uint32)
            for k, row in enumerate(("overlap", "n_excl", "n_match")):
                check(np.array_equal(got[k], want[label][k]), f"{name} {what}: {row} of {label} differs from run_device")

        # the reference rows, once: run_device on a handle of its own
        with RefDB(values, offsets) as h:
            h.set_lookup(_lib.YH_LOOKUP_INDEXED)
            want = {label: rows_plain(h, label) for label in smp}
        for size in SIZES:          # one sample per geometry against the CPU oracle
            label = f"clusters@{size}"
            ov = oracle.overlap(values, offsets, smp[label], threads=4)
            e, m = oracle.exclusive(values, offsets, ov > 0, smp[label])
            check(np.array_equal(want[label], np.stack([ov, np.where(ov > 0, e, 0), np.where(ov > 0, m, 0)])),
                  f"{name} run_device of {label} differs from the oracle")
            check(int((want[label][0] > 0).sum()) >= clustered.size, f"{name} {label}: the clustered references are not all hit")
            check(not want[f"miss@{size}"].any(), f"{name} miss@{size} hits something")

        for size in SIZES:
            lo, hi = f"miss@{size}", (f"all@{size}" if f"all@{size}" in smp else f"clusters@{size}")
            for nbuf in (3, 2):
                # swings from the first call of a fresh handle; rows read after exactly two further calls, no join
                with RefDB(values, offsets) as h:
                    h.set_lookup(_lib.YH_LOOKUP_INDEXED)
                    check(h.lookup_choice(size) == _lib.YH_LOOKUP_INDEXED, f"{name} {size}: the indexed lookup was not chosen")
                    bufs = [torch.empty((3, n), dtype=torch.int32, device=dev) for _ in range(nbuf)]
                    seq = [lo, hi, lo, hi, hi, lo, lo, hi, f"few@{size}", hi]
                    for b_ in bufs:
                        b_.fill_(-1)
                    torch.cuda.synchronize()
                    for i, label in enumerate(seq):
                        # (three buffers: the one of call i - 3 is complete and gets 0xFFFFFFFF again; two: the exclusive pass
                        # of call i - 2 still adds into the buffer in this very launch, so nothing may touch it)
                        call(h, label, bufs[i % nbuf], fill=nbuf == 3)
                        if i == 0:      # the launch is the fused one: this call's rows come with the calls behind it
                            torch.cuda.synchronize()
                            check(bool((bufs[0][0] == -1).all()), f"{name} {size}: the first pipelined call wrote its rows at once "
                                                                   "(not the fused launch)")
                        if i >= 2:      # complete after exactly two further calls (two buffers: call i itself has written nothing yet)
                            torch.cuda.synchronize()
                            same(bufs[(i - 2) % nbuf], seq[i - 2], f"{size} swings x{nbuf}, call {i - 2} read two calls later")
                    h.run_device_join()
                    h.synchronize()
                    same(bufs[(len(seq) - 1) % nbuf], seq[-1], f"{size} swings x{nbuf}, last call after the join")
                    if nbuf == 3:
                        same(bufs[(len(seq) - 2) % nbuf], seq[-2], f"{size} swings x3, last call but one after the join")
            with RefDB(values, offsets) as h:
                h.set_lookup(_lib.YH_LOOKUP_INDEXED)
                bufs = [torch.empty((3, n), dtype=torch.int32, device=dev) for _ in range(3)]
                # a join after one call, then after two
                call(h, hi, bufs[0])
                h.run_device_join()
                h.synchronize()
                same(bufs[0], hi, f"{size} join after one call")
                call(h, hi, bufs[0])
                call(h, lo, bufs[1])
                h.run_device_join()
                h.synchronize()
                same(bufs[0], hi, f"{size} join after two calls, first")
                same(bufs[1], lo, f"{size} join after two calls, second")
                # run_device in the middle of a pipeline: it joins first, and the pipeline starts again behind it
                call(h, hi, bufs[0])
                call(h, f"few@{size}", bufs[1])
                got = rows_plain(h, lo)
                check(np.array_equal(got, want[lo]), f"{name} {size}: run_device in the middle of a pipeline")
                same(bufs[0], hi, f"{size} rows in front of a run_device call, first")
                same(bufs[1], f"few@{size}", f"{size} rows in front of a run_device call, second")
                # set_stream in the middle of a pipeline: it joins; the next calls run on the new stream
                call(h, hi, bufs[0])
                call(h, lo, bufs[1])
                stream = torch.cuda.Stream()
                h.set_stream(stream.cuda_stream)
                torch.cuda.synchronize()
                same(bufs[0], hi, f"{size} rows in front of set_stream, first")
                same(bufs[1], lo, f"{size} rows in front of set_stream, second")
                for i, label in enumerate((hi, lo, hi)):
                    call(h, label, bufs[i])
                torch.cuda.synchronize()
                same(bufs[0], hi, f"{size} on the new stream, read two calls later")
                h.run_device_join()
                torch.cuda.synchronize()
                same(bufs[1], lo, f"{size} on the new stream, after the join")
                same(bufs[2], hi, f"{size} on the new stream, after the join, last")
                h.set_stream(0)


def _collect():
    failures, n_checks = [], [0]

    def check(ok, what):
        n_checks[0] += 1
        if not ok and len(failures) < 20:
            failures.append(what)

    scenarios(check)
    return failures, n_checks[0]


def test_fused_roles(hip_lib):
    failures, n_checks = _collect()
    assert n_checks > 200
    assert not failures, "\n".join(failures)


WORKER = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_fused_roles as t
failures, n_checks = t._collect()
print(json.dumps({"failures": failures, "checks": n_checks}))
"""


def test_fused_roles_one_exclusive_workgroup(hip_lib):
    """The exclusive role forced to its smallest size: one workgroup walks every list, the ones at capacity included."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("YH_")}
    env.update({"YH_DEBUG_TUNING": "1", "YH_FUSED_EXCL_WGS": "1"})
    r = subprocess.run([sys.executable, "-c", WORKER, ROOT], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] > 200
    assert not out["failures"], "\n".join(out["failures"])
