"""GPU: the streaming lookup (k_stream_lookup) at the edges of its blocks, runs of equal keys, tiles and sample ranges, every
comparison exact (np.array_equal against oracle.overlap / oracle.exclusive).

overlap, YH_LOOKUP_STREAM               the plain launch
run_counts, YH_LOOKUP_STREAM            the fused run step's launch (hits on shared hashes in a second replica set); with
                                        YH_NO_FUSED_RUN=1 the general one (hit flags by a search in the shared hashes)
overlap on a YH_DB_NO_INDEX handle      the stream and nothing else

The databases and samples are those of tests/stream_cases.py; which boundary each sits on under which environment is guarded
on the CPU by tests/test_stream_cases_cpu.py, which also pins the oracle's counts against a set-based count.  The expected
counts are computed once in this process and handed to the workers in a file.  For every database info()'s stream_layout,
stream_shift, stream_bytes and max_hash must equal the mirror's: a case that did not get its layout fails.

The tuning variables are read once per process: one child process per environment, each building each of its databases once.
    default             512 workgroups asked for: two or three blocks each on the 272- and 257-block databases
    wgs1, wgs2, wgs8,   YH_STREAM_WGS = 1, 2, 8, 9, 17, 19, 34, 39 behind YH_DEBUG_TUNING: 272 .. 7 blocks per workgroup, 16 .. 1
    wgs9 .. wgs39       per super-block (stream_cases.RANGES); the databases of three blocks run under default, wgs1, no_fused
    no_fused            the default geometry with YH_NO_FUSED_RUN=1
After a child that did not come back or died on a signal nothing more is started on the GPU.

Measured on an MI355X: about 2.5 s each for default, wgs1 and no_fused (all fourteen databases), 0.7 - 0.9 s for each of the
other seven environments (the 272-block database alone, wgs8 with the 256-block one) and 0.5 s for the expected counts: 14 s
for the file.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YH_DB_NO_INDEX = 1

_child_lost = []        # set by the first child that did not come back or died on a signal: nothing more is started on the GPU


def env_variables(env_name):
    wgs, no_fused = sc.ENVS[env_name]
    out = {}
    if wgs is not None:
        out["YH_STREAM_WGS"] = str(wgs)
    if no_fused:
        out["YH_NO_FUSED_RUN"] = "1"
    if out:
        out["YH_DEBUG_TUNING"] = "1"
    return out


def _sparse(out, key, rows):
    rows = np.asarray(rows, dtype=np.uint32)
    idx = np.flatnonzero(rows.any(axis=0))
    out[key + "idx"] = idx
    out[key + "val"] = rows[:, idx]


def _dense(exp, key, n):
    rows = np.zeros((3, n), dtype=np.uint32)
    rows[:, exp[key + "idx"]] = exp[key + "val"]
    return rows


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """The oracle's answers, once: "<case>/<sample label>/" the three count rows of the run step (n_excl and n_match zero
    outside the subset overlap > 0), stored as the non-zero columns."""
    from oracle import oracle

    out = {}
    for case in sc.all_cases():
        values, offsets = case.csr()
        for label, s in case.samples.items():
            ov = oracle.overlap(values, offsets, s)
            e, m = oracle.exclusive(values, offsets, ov > 0, s)
            _sparse(out, f"{case.name}/{label}/", np.stack([ov, np.where(ov > 0, e, 0), np.where(ov > 0, m, 0)]))
    path = str(tmp_path_factory.mktemp("stream_edges") / "expected.npz")
    np.savez(path, **out)
    return path


# ---- the child process ----------------------------------------------------------------------------------------------------
def worker(env_name, expected_path):
    """Runs in a child: every database of the environment built once (and once more without the index); prints one JSON line."""
    from yacht_amd import _lib
    from yacht_amd.engine import RefDB

    t_start = time.perf_counter()
    exp = np.load(expected_path)
    failures, built, n_checks, infos, per_case = [], [], [0], {}, {}

    def check(ok, *what):      # (what[0] = "<environment> <database>": the first few failures of every database are kept)
        n_checks[0] += 1
        if not ok:
            name = str(what[0])
            per_case[name] = per_case.get(name, 0) + 1
            if per_case[name] <= 6:
                failures.append(" ".join(str(w) for w in what))

    def at(*what):      # (where the child is, should it not come back)
        print("[stream edges]", env_name, *what, file=sys.stderr, flush=True)

    def info_of(h):
        i = h.info()
        return [int(i["stream_layout"]), int(i["stream_shift"]), int(i["stream_bytes"]), int(i["max_hash"])]

    for case in sc.cases_of(env_name):
        values, offsets = case.csr()
        n = case.n_refs
        lay = case.layout()
        mirror = [1, lay.sshift, lay.stream_bytes, lay.max_hash]
        tag = f"{env_name} {case.name}"
        at(case.name, "build")
        with RefDB(values, offsets) as h:
            built.append(case.name)
            infos[case.name] = info_of(h)
            check(infos[case.name] == mirror, tag, "stream_layout, stream_shift, stream_bytes, max_hash", infos[case.name], "mirror", mirror)
            h.set_lookup(_lib.YH_LOOKUP_STREAM)
            for label, s in case.samples.items():
                at(case.name, label)
                want = _dense(exp, f"{case.name}/{label}/", n)
                check(h.lookup_choice(s.size) == _lib.YH_LOOKUP_STREAM, tag, label, "the stream lookup was not chosen")
                ov = h.overlap(s)
                check(np.array_equal(ov, want[0]), tag, label, "overlap", _diff(ov, want[0]))
                got = h.run_counts(s)
                for k, name in enumerate(("overlap", "n_excl", "n_match")):
                    check(np.array_equal(got[k], want[k]), tag, label, "run_counts", name, _diff(got[k], want[k]))
        at(case.name, "build without the index")
        with RefDB(values, offsets, flags=YH_DB_NO_INDEX) as h:
            check(info_of(h) == mirror, tag, "no index: stream_layout, stream_shift, stream_bytes, max_hash", info_of(h), "mirror", mirror)
            for label, s in case.samples.items():
                at(case.name, label, "no index")
                want = _dense(exp, f"{case.name}/{label}/", n)
                check(h.lookup_choice(s.size) == _lib.YH_LOOKUP_STREAM, tag, label, "no index: the stream lookup was not chosen")
                ov = h.overlap(s)
                check(np.array_equal(ov, want[0]), tag, label, "no index: overlap", _diff(ov, want[0]))
    print(json.dumps({"built": built, "failures": failures, "failed_per_database": per_case, "checks": n_checks[0], "infos": infos,
                      "seconds": round(time.perf_counter() - t_start, 2)}))


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
import test_gpu_stream_edges as t
t.worker(sys.argv[2], sys.argv[3])
"""


@pytest.mark.parametrize("env_name", list(sc.ENVS))
def test_stream_edges(hip_lib, expected, env_name):
    assert not _child_lost, f"not started: the worker of {_child_lost[0]} did not come back or died on a signal"
    env = {k: v for k, v in os.environ.items() if not k.startswith("YH_")}
    env.update(env_variables(env_name))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-c", WORKER, ROOT, env_name, expected], capture_output=True, text=True, env=env, timeout=240)
    except subprocess.TimeoutExpired as e:
        _child_lost.append(env_name)
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("the worker did not come back; it was at:\n" + "\n".join(ln for ln in err.splitlines() if ln.startswith("[stream edges]"))[-600:])
    if r.returncode < 0 or (r.returncode != 0 and "illegal memory access" in r.stderr):
        _child_lost.append(env_name)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[stream edges] {env_name}: {out['checks']} checks, worker {out['seconds']} s, child {time.perf_counter() - t0:.2f} s")
    cases = sc.cases_of(env_name)
    assert out["built"] == [c.name for c in cases]
    for c in cases:      # the layout the case was written for
        lay = c.layout()
        assert out["infos"][c.name] == [1, lay.sshift, lay.stream_bytes, lay.max_hash], c.name
    assert out["checks"] == sum(2 + 7 * len(c.samples) for c in cases)
    assert not out["failures"], "\n".join(out["failures"] + [f"failed checks per database: {out['failed_per_database']}"])
