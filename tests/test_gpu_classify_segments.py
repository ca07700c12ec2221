"""RefDB.classify_segments (yh_classify_segments) on the GPU: from sequence to one row per record, the sketches never leaving
the device.  The rows must equal tests/classify_oracle.py on sketch.sketch_segments of the same buffer.

The database: 40 seeded random genomes of 20 kb at scaled 10 under a three-level tree (4 families x 2 genera x 5 species);
the species of a genus are point-mutated copies of its first one, so shared hashes exist at the genus level, and family 1's
second genus is derived from its first, so some resolve at the family; family 3's species are unrelated, so its records
resolve at a species.  The records: whole genomes, 2 kb and 150-base pieces
(some mutated), records of N's, records shorter than k, empty records, and a record made of halves of two genomes of different
families.

The first capacity for kept hashes is a tuning switch behind YH_DEBUG_TUNING=1, read once per process: the sizing retry runs
in a child process."""
import os
import subprocess
import sys

import lca_cases as cases
import numpy as np
import pytest
from classify_oracle import classify_oracle

from yacht_amd import sketch
from yacht_amd.engine import RefDB

pytestmark = pytest.mark.gpu

K = 31
SCALED = 10
NONE = 0xFFFFFFFF
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _random(rng, n):
    return BASES[rng.integers(0, 4, n)]


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(seq.size) < rate)
    out[at] = BASES[(np.searchsorted(BASES, seq[at]) + rng.integers(1, 4, at.size)) % 4]  # always another base
    return out


def _genomes(rng, n_bases=20_000):
    genomes, paths = [], []
    for f in range(4):
        first_of_family = None
        for g in range(2):
            if f == 1 and g == 1:
                base = _mutate(rng, first_of_family, 0.02)
            else:
                base = _random(rng, n_bases)
            if first_of_family is None:
                first_of_family = base
            for s in range(5):
                genomes.append(base if s == 0 else _random(rng, n_bases) if f == 3 else _mutate(rng, base, 0.01))
                paths.append((f"F{f}", f"F{f}g{g}", f"F{f}g{g}s{s}"))
    return genomes, paths


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    buf = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if seqs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8), off


def _database(rng, scaled, n_bases=20_000):
    genomes, paths = _genomes(rng, n_bases)
    mins, _ab, off = sketch.sketch_segments(*_pack(genomes), K, scaled)
    parent, depth, leaf = cases.tree_from_paths(paths)
    return genomes, mins, off, parent, depth, leaf


def _records(rng, genomes):
    recs = [genomes[0], genomes[7], genomes[39]]                                   # whole genomes
    for j in (1, 6, 12, 18, 25, 33):
        a = int(rng.integers(0, genomes[j].size - 2000))
        recs.append(genomes[j][a:a + 2000])                                        # 2 kb pieces
        recs.append(_mutate(rng, genomes[j][a:a + 2000], 0.03))                    # ... some mutated
    for j in rng.integers(0, len(genomes), 60):
        a = int(rng.integers(0, genomes[j].size - 150))
        piece = genomes[j][a:a + 150]
        recs.append(piece if j % 2 else _mutate(rng, piece, 0.02))                 # 150-base reads
    recs.append(np.full(500, ord("N"), dtype=np.uint8))                            # N's
    recs.append(np.zeros(0, dtype=np.uint8))                                       # empty
    recs.append(genomes[3][:K - 1])                                                # shorter than k
    recs.append(np.concatenate([genomes[2][:10_000], genomes[31][10_000:]]))       # halves of two families
    recs.append(_random(rng, 3000))                                                # in no genome
    recs.append(np.zeros(0, dtype=np.uint8))
    recs.append(np.full(40, ord("N"), dtype=np.uint8))
    recs.append(genomes[11][5000:5000 + K])                                        # exactly one window
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


@pytest.fixture(scope="module")
def world(hip_lib):
    rng = np.random.default_rng(2024)
    genomes, mins, off, parent, depth, leaf = _database(rng, SCALED)
    recs = _records(rng, genomes)
    buf, seg_off = _pack(recs)
    s_mins, _ab, s_off = sketch.sketch_segments(buf, seg_off, K, SCALED)
    want, nodes = classify_oracle(mins, off, parent, leaf, s_mins, s_off)
    return dict(genomes=genomes, mins=mins, off=off, parent=parent, depth=depth, leaf=leaf, recs=recs, buf=buf, seg_off=seg_off,
                s_mins=s_mins, s_off=s_off, want=want, nodes=nodes)


def _eq(got, want, what):
    for f in ("node", "n_kept", "n_hit", "n_root"):
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, bad[:10], got[bad[:10]], want[bad[:10]])


def test_rows_from_sequence_equal_the_oracle_on_the_sketches(world):
    w = world
    want = w["want"]
    depth = w["depth"]
    # the cases hold what they are meant to hold
    assert (want["n_kept"] == 0).sum() >= 5 and ((want["n_kept"] > 0) & (want["n_hit"] == 0)).sum() >= 1
    known = want[(want["node"] != NONE)]
    assert {int(depth[v]) for v in known["node"]} >= {0, 1, 2, 3}  # the root (two families), a family, genera, species
    assert w["s_mins"].size > 1024  # more than one tile of entries
    with RefDB(w["mins"], w["off"]) as db:
        assert db.info()["n_shared_distinct"] > 100
        db.set_taxonomy(w["parent"], w["depth"], w["leaf"])
        rows, total = db.classify_segments(w["buf"], w["seg_off"], K, SCALED, return_total=True)
        assert total == w["s_mins"].size
        _eq(rows, want, "segments")
        assert db.classify_segments(w["buf"].tobytes(), w["seg_off"], K, SCALED).tobytes() == rows.tobytes()
        _eq(db.classify_sets(w["s_mins"], w["s_off"]), want, "the same sketches as sets")
        # touching segments without a separator: the rows of the same records sketched alone
        for s in (0, 5, 17, len(w["recs"]) - 1, int(np.argmax(want["n_kept"]))):
            alone = db.classify_segments(w["recs"][s], np.array([0, w["recs"][s].size], np.uint64), K, SCALED)
            assert alone.tolist() == [rows[s].tolist()], s
        # no record, one empty record, only records without a window
        assert db.classify_segments(np.zeros(0, np.uint8), np.zeros(1, np.uint64), K, SCALED).size == 0
        assert db.classify_segments(np.zeros(0, np.uint8), np.zeros(2, np.uint64), K, SCALED).tolist() == [(NONE, 0, 0, 0)]
        short = db.classify_segments(w["genomes"][0][:40], np.array([0, 20, 20, 40], np.uint64), K, SCALED)
        assert short.tolist() == [(NONE, 0, 0, 0)] * 3
        from yacht_amd import _lib
        for bad_off in ([0, 10], [1, w["buf"].size], [0, 30, 20, w["buf"].size]):  # seg_off is validated
            with pytest.raises(_lib.YachtHipError) as e:
                db.classify_segments(w["buf"], np.array(bad_off, np.uint64), K, SCALED)
            assert e.value.code == _lib.YH_ERR_INVALID_ARG
        with pytest.raises(_lib.YachtHipError) as e:  # a max_hash below the database's largest hash is not its own
            db.classify_segments(w["buf"], w["seg_off"], K, 1000)
        assert e.value.code == _lib.YH_ERR_INVALID_ARG
        db.set_taxonomy(None, None, None)
        with pytest.raises(_lib.YachtHipError) as e:
            db.classify_segments(w["buf"], w["seg_off"], K, SCALED)
        assert e.value.code == _lib.YH_ERR_UNSUPPORTED


def _retry_case():
    """Child process: scaled 1 keeps every window; a first capacity of 1 000 pairs makes the call size itself again."""
    rng = np.random.default_rng(7)
    genomes, mins, off, parent, depth, leaf = _database(rng, 1, n_bases=600)
    recs = [genomes[0], genomes[5][100:400], np.zeros(0, np.uint8), _mutate(rng, genomes[12], 0.05), genomes[39], _random(rng, 700),
            np.concatenate([genomes[1][:300], genomes[30][300:]])]
    buf, seg_off = _pack(recs)
    s_mins, _ab, s_off = sketch.sketch_segments(buf, seg_off, K, 1)
    assert s_mins.size > 3000  # three times the first capacity
    want, _nodes = classify_oracle(mins, off, parent, leaf, s_mins, s_off)
    with RefDB(mins, off) as db:
        db.set_taxonomy(parent, depth, leaf)
        rows, total = db.classify_segments(buf, seg_off, K, 1, return_total=True)
    assert total == s_mins.size, (total, s_mins.size)
    _eq(rows, want, "retry")
    assert (want["n_hit"] > 0).sum() >= 5
    print("retry ok", total)


def test_sizing_retry_at_scaled_one(hip_lib):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, YH_DEBUG_TUNING="1", YH_CLASSIFY_FIRST_CAP="1000")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_classify_segments as t; t._retry_case()"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=here)
    assert p.returncode == 0 and "retry ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
