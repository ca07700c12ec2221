"""GPU: the exclusive pass behind the lookups at the edges of its holder-set records, pieces, work-list blocks and subset
words, every comparison exact (np.array_equal against oracle.overlap / oracle.exclusive).

run_counts, indexed and stream lookup   k_reduce_replicas with the work list, k_excl_pieces over the holder sets (U = 4)
run_device_pipelined x 3 + join         reduce_replicas_multi<4> and the U = 2 exclusive role of k_step_fused, three step contexts
exclusive(mask, sample)                 k_excl_worklist, k_excl_pieces over the postings with hit flags, k_excl_final
run_batch                               k_batch_maskwords, k_batch_worklist, k_batch_sets, k_batch_final_sparse (k_batch_final with
                                        YH_BATCH_DENSE_FINAL=1); run_batch_rows_pack_device / _unpack_device reproduce the dense rows

The databases, samples, masks and batch blocks are those of tests/excl_cases.py (what state each reaches is guarded on the CPU
by tests/test_excl_cases_cpu.py, which also pins the oracle's counts against a second computation); the expected counts are
computed once in this process and handed to the workers in a file.  Every *_device entry finds 0xFFFFFFFF in each output
buffer it must overwrite.  For every database n_holder_sets and n_shared_postings must equal the mirror's and the directory
must have taken the compact form (without it the pipelined step is not the fused launch): a case that did not reach its form
fails.

The tuning variables are read once per process: one child process per environment, each building each of its databases once.
    default        everything
    no_fused       YH_NO_FUSED_RUN=1: the run step through the general pass
    dense_final    YH_BATCH_DENSE_FINAL=1: the batch's dense final pass
    lanes1024      the work-list and the two 393 k databases with samples widened to 262 144 hashes by hashes nobody holds: the
                   size from which k_step_fused runs 1024 lanes and its reducer takes blocks of 4096 references (the fused
                   launch's geometry follows the sample's size; YH_INDEX_TILE=1 gives the stand-alone lookup the same lanes)
After a child that did not come back or died on a signal nothing more is started on the GPU.

Measured on an MI355X: about 3.4 s (default), 2.8 s (no_fused), 2.7 s (dense_final), 2.6 s (lanes1024) and 0.5 s for the
expected counts: 12.4 s for the file, most of it the four children's start.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import excl_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = {
    # name: (variables, case names (None: all), consumers)
    "default": ({}, None, ("run", "pipelined", "exclusive", "batch", "blocks")),
    "no_fused": ({"YH_NO_FUSED_RUN": "1"}, None, ("run", "pipelined")),
    "dense_final": ({"YH_BATCH_DENSE_FINAL": "1"}, None, ("batch", "blocks")),
    "lanes1024": ({"YH_INDEX_TILE": "1"}, tuple(c.name for c in ec.cases_work() + ec.cases_big()), ("padded",)),
}
BIG = tuple(c.name for c in ec.cases_big())

_child_lost = []        # set by the first child that did not come back or died on a signal: nothing more is started on the GPU


def cases_of(env_name):
    names = ENVS[env_name][1]
    return [c for c in ec.all_cases() if names is None or c.name in names]


def sample_labels(case):
    """The samples a database is asked with: all of a small one's; of a 393 k one its subsets', the shared and the noise sample."""
    return list(case.samples())


def padded_labels(case):
    """The samples of the 1024-lane environment (three steps are in flight together; a last group is filled up by repeating)."""
    if case.name in BIG:
        return ["P:both_sides", "P:last_words", "P:k9_high_alone", "shared"]
    return ["P:everyone", "P:only_last", "shared"]


def batch_labels(case):
    return ["P:both_sides", "shared"] if case.name in BIG else sample_labels(case)


def _sparse(out, key, rows):
    rows = np.asarray(rows, dtype=np.uint32)
    idx = np.flatnonzero(rows.any(axis=0))
    out[key + "idx"] = idx
    out[key + "val"] = rows[:, idx]


def _dense(exp, key, n):
    rows = np.zeros(exp[key + "val"].shape[:1] + (n,), dtype=np.uint32)
    rows[:, exp[key + "idx"]] = exp[key + "val"]
    return rows


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """The oracle's answers, once: "<case>/<sample label>/" the three count rows of the run step (zero outside the subset, as
    tests/test_gpu_batch.py::_want has it), "<case>/M:<mask label>/" the two rows of exclusive, "<case>/pad:<label>/" the run
    step's on the widened sample, "<case>/B:<label>/" the batch blocks' samples; stored as the non-zero columns."""
    from oracle import oracle

    def run_rows(values, offsets, s, threads):
        ov = oracle.overlap(values, offsets, s, threads=threads)
        e, m = oracle.exclusive(values, offsets, ov > 0, s)
        return np.stack([ov, np.where(ov > 0, e, 0), np.where(ov > 0, m, 0)])

    out = {}
    for case in ec.all_cases():
        values, offsets = case.csr()
        threads = 8 if case.n_refs > 100_000 else 1
        smp = case.samples()
        for label in sample_labels(case):
            _sparse(out, f"{case.name}/{label}/", run_rows(values, offsets, smp[label], threads))
        for label, mask, sample_label in case.masks():
            _sparse(out, f"{case.name}/M:{label}/", np.stack(oracle.exclusive(values, offsets, mask, smp[sample_label])))
        if case.name in ENVS["lanes1024"][1]:
            for label in padded_labels(case):
                _sparse(out, f"{case.name}/pad:{label}/", run_rows(values, offsets, ec.padded(case, smp[label]), threads))
    for case in ec.batch_cases():
        values, offsets = case.csr()
        for label, s in ec.batch_samples(case).items():
            _sparse(out, f"{case.name}/B:{label}/", run_rows(values, offsets, s, 1))
    path = str(tmp_path_factory.mktemp("excl_edges") / "expected.npz")
    np.savez(path, **out)
    return path


# ---- the child process ----------------------------------------------------------------------------------------------------
def worker(env_name, expected_path):
    """Runs in a child: every database of the environment built once, every consumer of the environment; prints one JSON line."""
    import torch

    from yacht_amd import _lib
    from yacht_amd.engine import RefDB, pack_csr

    _env, _names, consumers = ENVS[env_name]
    exp = np.load(expected_path)
    failures, built, n_checks, infos, per_case = [], [], [0], {}, {}
    dev = "cuda"

    def check(ok, *what):      # (what[0] = "<environment> <database> ...": the first few failures of every database are kept)
        n_checks[0] += 1
        if not ok:
            name = " ".join(str(what[0]).split()[:2])
            per_case[name] = per_case.get(name, 0) + 1
            if per_case[name] <= 6:
                failures.append(" ".join(str(w) for w in what))

    def at(*what):      # (where the child is, should it not come back)
        print("[excl edges]", env_name, *what, file=sys.stderr, flush=True)

    def rows3(tag, what, got, want):
        for k, name in enumerate(("overlap", "n_excl", "n_match")):
            check(np.array_equal(got[k], want[k]), tag, what, name, _diff(got[k], want[k]))

    def pipelined(h, case, n, labels, smp_of, key_of, tag):
        """Three steps in flight and the join; each output buffer holds 0xFFFFFFFF before its step."""
        outs = [torch.zeros((3, n), dtype=torch.int32, device=dev) for _ in range(3)]
        h.set_lookup(_lib.YH_LOOKUP_INDEXED)
        for g in range(0, len(labels), 3):
            group = [labels[min(g + i, len(labels) - 1)] for i in range(3)]
            bufs = []
            for o, label in zip(outs, group):       # (a step reads its sample when it runs: one buffer per step in flight)
                s = smp_of(label)
                bufs.append((torch.from_numpy(s.view(np.int64).copy()).to(dev), s.size))
                o.fill_(-1)
            torch.cuda.synchronize()
            for o, (b, size) in zip(outs, bufs):
                check(h.lookup_choice(size) == _lib.YH_LOOKUP_INDEXED, tag, "pipelined: the indexed lookup was not chosen")
                h.run_device_pipelined(b.data_ptr(), size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
            h.run_device_join()
            h.synchronize()
            for i, (o, label) in enumerate(zip(outs, group)):
                rows3(tag, f"pipelined step {i} of {group} ({label})", o.cpu().numpy().view(np.uint32), _dense(exp, key_of(label), n))
        h.set_lookup(_lib.YH_LOOKUP_AUTO)

    def batch_device(h, case, n, samples, wants, tag):
        """run_batch_device into buffers of 0xFFFFFFFF, then the compact rows: they must reproduce the dense ones."""
        b = len(samples)
        values, offsets = pack_csr(samples)
        d_v = torch.from_numpy(np.concatenate([values, np.zeros(1, np.uint64)]).view(np.int64).copy()).to(dev)
        d_o = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        out = torch.full((3, b, n), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h.run_batch_device(d_v.data_ptr(), d_o.data_ptr(), b, int(values.size), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        h.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        for j in range(b):
            rows3(tag, f"batch_device sample {j} of {b}", got[:, j], wants[j])
        entries = int(sum(int((w[0] > 0).sum()) for w in wants))
        cap = entries + 8
        vals = torch.full((cap, 3), -1, dtype=torch.int32, device=dev)
        rows = torch.full((cap, 5), -1, dtype=torch.int32, device=dev)
        n1 = torch.full((1,), -1, dtype=torch.int32, device=dev)
        n2 = torch.full((1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h.run_batch_rows_pack_device(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), vals.data_ptr(), cap, n1.data_ptr())
        h.run_batch_rows_unpack_device(vals.data_ptr(), cap, rows.data_ptr(), n2.data_ptr())
        h.synchronize()
        k = int(n1.item())
        check(k == int(n2.item()) == entries, tag, "batch rows: entries", k, int(n2.item()), "want", entries)
        if k == entries:
            r = rows[:k].cpu().numpy().view(np.uint32)
            dense = np.zeros((3, b, n), dtype=np.uint32)
            for c in range(3):
                dense[c, r[:, 0], r[:, 1]] = r[:, 2 + c]
            check(np.array_equal(dense, np.stack(wants, axis=1)), tag, "batch rows do not reproduce the dense rows")
            check(np.array_equal(np.lexsort((r[:, 0], r[:, 1])), np.arange(k)), tag, "batch rows: (reference, sample) order")

    for case in cases_of(env_name):
        values, offsets = case.csr()
        n = case.n_refs
        smp = case.samples()
        mir = case.mirror()
        at(case.name, "build")
        with RefDB(values, offsets) as h:
            built.append(case.name)
            info = h.info()
            infos[case.name] = [int(info["n_holder_sets"]), int(info["n_shared_postings"])]
            check(infos[case.name] == [mir.n_holder_sets(), mir.n_shared_postings], f"{env_name} {case.name}", "n_holder_sets, n_shared_postings",
                  infos[case.name], "mirror", [mir.n_holder_sets(), mir.n_shared_postings])
            tag = f"{env_name} {case.name}"
            labels = sample_labels(case)
            if "run" in consumers:
                for label in labels:
                    at(case.name, label, "run")
                    want = _dense(exp, f"{case.name}/{label}/", n)
                    for mode, name in ((_lib.YH_LOOKUP_INDEXED, "indexed"), (_lib.YH_LOOKUP_STREAM, "stream")):
                        h.set_lookup(mode)
                        check(h.lookup_choice(smp[label].size) == mode, tag, label, name, "lookup was not chosen")
                        rows3(tag, f"{label} run_counts {name}", h.run_counts(smp[label]), want)
                    h.set_lookup(_lib.YH_LOOKUP_AUTO)
            if "pipelined" in consumers:
                at(case.name, "pipelined")
                pipelined(h, case, n, labels, lambda label: smp[label], lambda label: f"{case.name}/{label}/", tag)
            if "padded" in consumers:
                wide = {label: ec.padded(case, smp[label]) for label in padded_labels(case)}
                h.set_lookup(_lib.YH_LOOKUP_INDEXED)
                for label, s in wide.items():
                    at(case.name, label, "padded run")
                    rows3(tag, f"pad:{label} run_counts indexed", h.run_counts(s), _dense(exp, f"{case.name}/pad:{label}/", n))
                h.set_lookup(_lib.YH_LOOKUP_AUTO)
                at(case.name, "padded pipelined")
                pipelined(h, case, n, list(wide), lambda label: wide[label], lambda label: f"{case.name}/pad:{label}/", tag + " padded")
            if "exclusive" in consumers:
                for label, mask, sample_label in case.masks():
                    at(case.name, label, "exclusive")
                    want = _dense(exp, f"{case.name}/M:{label}/", n)
                    e, m = h.exclusive(mask, smp[sample_label])
                    check(np.array_equal(e, want[0]), tag, "exclusive", label, "n_excl", _diff(e, want[0]))
                    check(np.array_equal(m, want[1]), tag, "exclusive", label, "n_match", _diff(m, want[1]))
            if "batch" in consumers:
                bl = batch_labels(case)
                for g in range(0, len(bl), 256):
                    at(case.name, "batch", g)
                    group = bl[g: g + 256]
                    wants = [_dense(exp, f"{case.name}/{label}/", n) for label in group]
                    got = h.run_batch([smp[label] for label in group])
                    for j, label in enumerate(group):
                        rows3(tag, f"run_batch {label} at {j} of {len(group)}", [got[k][j] for k in range(3)], wants[j])
                    if g == 0:
                        few = group if n > 100_000 else group[:70]
                        batch_device(h, case, n, [smp[label] for label in few], wants[: len(few)], tag)
            if "blocks" in consumers and case.name in [c.name for c in ec.batch_cases()]:
                bs = ec.batch_samples(case)
                for b in ec.BATCH_B:
                    at(case.name, "block of", b)
                    block = ec.batch_block(case, b)
                    wants = [_dense(exp, f"{case.name}/B:{label}/", n) for label in block]
                    got = h.run_batch([bs[label] for label in block])
                    for j, label in enumerate(block):
                        rows3(tag, f"block of {b}: {label} at {j}", [got[k][j] for k in range(3)], wants[j])
                    batch_device(h, case, n, [bs[label] for label in block], wants, f"{tag} block of {b}")
    print(json.dumps({"built": built, "failures": failures, "failed_per_database": per_case, "checks": n_checks[0], "infos": infos}))


def _diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.flatnonzero((got != want).reshape(-1))
    if not bad.size:
        return ""
    return f"{bad.size} differ, first at {int(bad[0])}: got {got.reshape(-1)[bad[0]]}, want {want.reshape(-1)[bad[0]]}"


WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_excl_edges as t
t.worker(sys.argv[2], sys.argv[3])
"""


@pytest.mark.parametrize("env_name", list(ENVS))
def test_exclusive_edges(hip_lib, expected, env_name):
    assert not _child_lost, f"not started: the worker of {_child_lost[0]} did not come back or died on a signal"
    variables, _names, consumers = ENVS[env_name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("YH_")}
    env.update({"YH_DEBUG_TUNING": "1", "YH_TRACE_BUILD": "1"})
    env.update(variables)
    try:
        r = subprocess.run([sys.executable, "-c", WORKER, ROOT, env_name, expected], capture_output=True, text=True, env=env, timeout=240)
    except subprocess.TimeoutExpired as e:
        _child_lost.append(env_name)
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("the worker did not come back; it was at:\n" + "\n".join(ln for ln in err.splitlines() if ln.startswith("[excl edges]"))[-600:])
    if r.returncode < 0 or (r.returncode != 0 and "illegal memory access" in r.stderr):
        _child_lost.append(env_name)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    cases = cases_of(env_name)
    assert out["built"] == [c.name for c in cases]
    # every database took the compact directory form (what the fused launch needs) and the mirror's record and posting counts
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[yh build] directory form ")]
    assert len(lines) == len(cases) and all(ln.startswith("[yh build] directory form compact: ") for ln in lines), r.stderr[-2000:]
    for c in cases:
        assert out["infos"][c.name] == [c.mirror().n_holder_sets(), c.mirror().n_shared_postings], c.name
    assert out["checks"] > 6 * len(cases)
    assert not out["failures"], "\n".join(out["failures"] + [f"failed checks per database: {out['failed_per_database']}"])
