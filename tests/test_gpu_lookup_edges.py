"""GPU: the five kernels that read the directory over the database's distinct hashes (YhDirView) at the edges of its three
bucket forms, every comparison exact.

k_index_lookup_tile   run_counts and overlap with the indexed lookup forced, in its four geometries (YH_INDEX_TILE = 256, 1, 2, 4)
k_step_fused          run_device_pipelined three times + run_device_join with the indexed lookup forced, in the small and both
                      1024-lane geometries (where yh_q_step_fused_ok does not hold -- wide forms, no shared hash -- the call
                      falls back to the plain indexed step; the counts hold there too)
k_batch_lookup        run_batch with the sample alone, as one of 3 with an empty one in between, as one of 65
k_abund_lookup        abundance with random abundances (small cases: also all 2^32 - 1)
k_explain_lookup      explain with random seven-bit member bytes: flags and totals

The databases and samples are those of tests/lookup_cases.py (what state each reaches is guarded on the CPU by
tests/test_lookup_cases_cpu.py); the expected counts come from the oracles (oracle.overlap / oracle.exclusive,
tests/abund_oracle.py, tests/explain_oracle.py), computed once in this process and handed to the workers in a file.

The tuning variables are read once per process, so the work is grouped into one child process per environment: each builds
each of its databases once, runs every consumer and reports what differed.  From the build's trace line every child's
databases must have taken the intended form, with the intended bucket count, multiplier, overflow entries and capacity and
filter size (all stated by the plain-int mirror in lookup_cases.py): a case that did not reach its form fails.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lookup_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER = {"YH_FILTER_MIN": "1"}
ENVS = {
    # name: (variables, databases (None: all), samples of the indexed consumers, samples of the other consumers)
    "default": ({}, None, "all", "all"),
    "tile256": ({"YH_INDEX_TILE": "256"}, None, "all", "none"),
    "tile1_filter1": ({"YH_INDEX_TILE": "1", "YH_FILTER_BPH": "1", **FILTER}, None, "all", "padded"),
    "tile2_filter4": ({"YH_INDEX_TILE": "2", "YH_FILTER_BPH": "4", **FILTER}, None, "all", "padded"),
    "tile4_filter16": ({"YH_INDEX_TILE": "4", "YH_FILTER_BPH": "16", **FILTER}, None, "all", "padded"),
    "tile2_no_filter": ({"YH_INDEX_TILE": "2", "YH_NO_FILTER": "1", **FILTER}, None, "all", "padded"),
    "wide_buckets": ({"YH_WIDE_BUCKETS": "1"}, ("compact_edge",), "all", "all"),
    "no_buckets": ({"YH_NO_BUCKETS": "1"}, ("wide_full", "wide_edge", "wide_four"), "all", "all"),
}
OTHERS = (2047, 2048, 2049)        # the other samples of a batch: prefixes around the batch tile
ALL_ONES = 2 ** 32 - 1


_child_lost = []        # set by the first child that did not come back or died on a signal: nothing more is started on the GPU


def gpu_databases():
    return list(lc.databases())


def _seed(*parts):
    return [sum(ord(c) for c in p) for p in parts]


def abundances(name, label, n):
    return np.random.default_rng(_seed(name, label)).integers(1, 1001, size=n).astype(np.uint32)


def members(name, n_refs):
    return np.random.default_rng(_seed(name, "members")).integers(0, 128, size=n_refs).astype(np.uint8)


def _small(db):
    return db.name.startswith("small_")


def _others(forms):
    return [forms.get(f"prefix_{n}", forms["base"]) for n in OTHERS]


def _other_labels(forms):
    return [f"prefix_{n}" if f"prefix_{n}" in forms else "base" for n in OTHERS]


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """The oracles' answers for every (database, sample), once: a file of arrays "<database>/<sample>/<what>"."""
    from abund_oracle import abundance_oracle
    from explain_oracle import explain_oracle, totals_from_flags
    from oracle import oracle

    out = {}
    for db in gpu_databases():
        values, offsets = db.csr()
        member = members(db.name, db.n_refs)
        for label, s in lc.samples(db.name).items():
            key = f"{db.name}/{label}/"
            ov = oracle.overlap(values, offsets, s)
            e, m = oracle.exclusive(values, offsets, ov > 0, s)
            out[key + "counts"] = np.stack([ov, e, m])
            ab = abundances(db.name, label, s.size)
            w_ov, w_m, med = abundance_oracle(values, offsets, s, ab)
            out[key + "abund"] = np.stack([w_ov, w_m])
            out[key + "median"] = med
            if _small(db) and not label.startswith("padded"):
                w_ov, w_m, med = abundance_oracle(values, offsets, s, np.full(s.size, ALL_ONES, dtype=np.uint64))
                out[key + "abund_ones"] = np.stack([w_ov, w_m])
                out[key + "median_ones"] = med
            flags, _ = explain_oracle(values, offsets, s, member)
            out[key + "flags"] = flags
            out[key + "totals"] = totals_from_flags(flags, ab)
    path = str(tmp_path_factory.mktemp("lookup_edges") / "expected.npz")
    np.savez(path, **out)
    return path


# ---- the child process ----------------------------------------------------------------------------------------------------
def worker(env_name, expected_path):
    """Runs in a child: every database of the environment built once, every consumer on every sample; prints one JSON line."""
    import torch

    from yacht_amd import _lib
    from yacht_amd.engine import RefDB

    _env, names, indexed_on, others_on = ENVS[env_name]
    exp = np.load(expected_path)
    failures, built, n_checks = [], [], [0]

    d_sample = torch.zeros(lc.PADDED[-1], dtype=torch.int64, device="cuda")      # every sample is copied into this one buffer

    def check(ok, *what):
        n_checks[0] += 1
        if not ok and len(failures) < 60:
            failures.append(" ".join(str(w) for w in what))

    def wanted(which, label):
        return which == "all" or (which == "padded" and label.startswith("padded"))

    def at(*what):      # (where the child is, should it not come back)
        print("[lookup edges]", env_name, *what, file=sys.stderr, flush=True)

    for db in gpu_databases():
        if names is not None and db.name not in names:
            continue
        values, offsets = db.csr()
        n = db.n_refs
        forms = lc.samples(db.name)
        member = members(db.name, n)
        other_labels = _other_labels(forms)
        other_samples = _others(forms)
        at(db.name, "build")
        with RefDB(values, offsets) as h:
            built.append(db.name)
            outs = [torch.zeros((3, n), dtype=torch.int32, device="cuda") for _ in range(3)]
            for label, s in forms.items():
                key = f"{db.name}/{label}/"
                tag = f"{env_name} {db.name} {label}"
                want = exp[key + "counts"]
                at(db.name, label)
                if wanted(indexed_on, label):       # k_index_lookup_tile
                    h.set_lookup(_lib.YH_LOOKUP_INDEXED)
                    check(h.lookup_choice(s.size) == _lib.YH_LOOKUP_INDEXED, tag, "the indexed lookup was not chosen")
                    got = h.run_counts(s)
                    for k, what in enumerate(("overlap", "n_excl", "n_match")):
                        check(np.array_equal(got[k], want[k]), tag, "run_counts", what, _diff(got[k], want[k]))
                    got = h.overlap(s)
                    check(np.array_equal(got, want[0]), tag, "overlap", _diff(got, want[0]))
                    h.set_lookup(_lib.YH_LOOKUP_AUTO)
                if not wanted(others_on, label):
                    continue
                # k_step_fused: three pipelined steps and the join.  The indexed lookup stays forced: left to the cost model, a small
                # database asked with a large sample goes to the stream lookup instead, which is not what this file is about
                at(db.name, label, "pipelined")
                d_sample[: s.size].copy_(torch.from_numpy(s.view(np.int64).copy()))
                for o in outs:
                    o.zero_()
                torch.cuda.synchronize()
                h.set_lookup(_lib.YH_LOOKUP_INDEXED)
                check(h.lookup_choice(s.size) == _lib.YH_LOOKUP_INDEXED, tag, "pipelined: the indexed lookup was not chosen")
                for o in outs:
                    h.run_device_pipelined(d_sample.data_ptr(), s.size, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
                h.run_device_join()
                h.synchronize()
                h.set_lookup(_lib.YH_LOOKUP_AUTO)
                for i, o in enumerate(outs):
                    got = o.cpu().numpy().view(np.uint32)
                    check(np.array_equal(got, want), tag, "pipelined step", i, _diff(got, want))
                # k_batch_lookup: alone, one of 3 around an empty sample, one of 65
                at(db.name, label, "batch")
                empty = np.zeros(0, dtype=np.uint64)
                zero = np.zeros((3, n), dtype=np.uint32)
                w_other = [exp[f"{db.name}/{ol}/counts"] for ol in other_labels]
                many = [other_samples[i % 3] for i in range(65)]
                many[37] = s
                w_many = [w_other[i % 3] for i in range(65)]
                w_many[37] = want
                for what, batch, w in (("alone", [s], [want]), ("of 3", [other_samples[0], empty, s], [w_other[0], zero, want]),
                                       ("of 65", many, w_many)):
                    got = h.run_batch(batch)
                    for j in range(len(batch)):
                        for k in range(3):
                            check(np.array_equal(got[k][j], w[j][k]), tag, "batch", what, "sample", j, "row", k, _diff(got[k][j], w[j][k]))
                # k_abund_lookup
                at(db.name, label, "abundance")
                ab = abundances(db.name, label, s.size)
                rounds = [(ab, "abund", "median")]
                if key + "abund_ones" in exp:
                    rounds.append((np.full(s.size, ALL_ONES, dtype=np.uint64), "abund_ones", "median_ones"))
                for a, ka, km in rounds:
                    w_ov, w_m, med = h.abundance(s, a)
                    check(np.array_equal(w_ov, exp[key + ka][0]), tag, ka, "w_overlap", _diff(w_ov, exp[key + ka][0]))
                    check(np.array_equal(w_m, exp[key + ka][1]), tag, ka, "w_match", _diff(w_m, exp[key + ka][1]))
                    check(np.array_equal(med, exp[key + km]), tag, km, _diff(med, exp[key + km]))
                # k_explain_lookup
                at(db.name, label, "explain")
                flags, totals = h.explain(s, member, ab)
                check(np.array_equal(flags, exp[key + "flags"]), tag, "explain flags", _diff(flags, exp[key + "flags"]))
                check(np.array_equal(totals, exp[key + "totals"]), tag, "explain totals")
    print(json.dumps({"built": built, "failures": failures, "checks": n_checks[0]}))


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
import test_gpu_lookup_edges as t
t.worker(sys.argv[2], sys.argv[3])
"""


def _intended(db, variables):
    """The trace line the build must print for db under the environment's variables (from the mirror)."""
    g = db.geometry(wide_buckets=variables.get("YH_WIDE_BUCKETS") == "1", no_buckets=variables.get("YH_NO_BUCKETS") == "1")
    n_over = cap = fbits = 0
    if g.form == "compact":
        n_over = len(lc.overflow_entries(db.distinct, g))
        cap = lc.ovf_capacity(n_over)
        if variables.get("YH_FILTER_MIN") == "1":
            fbits = lc.filter_geometry(g, int(variables["YH_FILTER_BPH"]) if "YH_FILTER_BPH" in variables else 4)[0]
    return f"[yh build] directory form {g.form}: nb {g.nb} mul {g.mul} overflow {n_over} of {cap} filter bits {fbits}"


@pytest.mark.parametrize("env_name", list(ENVS))
def test_directory_edges(hip_lib, expected, env_name):
    assert not _child_lost, f"not started: the worker of {_child_lost[0]} did not come back or died on a signal"
    variables, names, _indexed_on, _others_on = ENVS[env_name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("YH_")}
    env.update({"YH_DEBUG_TUNING": "1", "YH_TRACE_BUILD": "1"})
    env.update(variables)
    try:
        r = subprocess.run([sys.executable, "-c", WORKER, ROOT, env_name, expected], capture_output=True, text=True, env=env, timeout=180)
    except subprocess.TimeoutExpired as e:
        _child_lost.append(env_name)
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("the worker did not come back; it was at:\n" + "\n".join(ln for ln in err.splitlines() if ln.startswith("[lookup edges]"))[-600:])
    if r.returncode < 0:
        _child_lost.append(env_name)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    dbs = [db for db in gpu_databases() if names is None or db.name in names]
    assert out["built"] == [db.name for db in dbs]
    # the form every database took, from the build's trace line
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[yh build] directory form ")]
    assert lines == [_intended(db, variables) for db in dbs], r.stderr[-2000:]
    if env_name == "default":
        assert [ln.split()[4].rstrip(":") for ln in lines] == [db.form for db in dbs]
        by = dict(zip(out["built"], lines))
        assert by["overflow_504"].endswith("overflow 504 of 1024 filter bits 0") and by["overflow_505"].endswith("overflow 505 of 2048 filter bits 0")
        assert " nb 4096 mul 4096 " in by["compact_edge"] and " form wide: nb 5119 " in by["wide_edge"]
    if env_name == "wide_buckets":
        assert lines[0].startswith("[yh build] directory form wide: nb 5119 mul 5119 ")
    if env_name == "no_buckets":
        assert all(ln.startswith("[yh build] directory form directory: nb 0 ") for ln in lines)
    if "YH_FILTER_BPH" in variables:
        assert all(not ln.endswith(" filter bits 0") for ln in lines if " form compact: " in ln)      # (only the compact form has one)
    assert out["checks"] > 20 * len(dbs)
    assert not out["failures"], "\n".join(out["failures"])
