"""GPU: the three kernels of yh_pack.hip at the edges of their formats, every comparison exact.

k_unpack_sample   packed samples of every block width 0..64, wide gaps at the lanes around the wave boundaries, block tails of
                  1, 2, 63, 64, 65, 255 and 256 hashes, runs at the top of the range (tests/packed_cases.py).  The library has no
                  call that returns the expanded sample, so every expanded hash is observed through the lookup: the database is
                  made of the sample itself -- whole, block by block, and the hashes whose lane has bit t set, t = 0..7.  The
                  overlap of each of these references must be its size; with the kernel's own ordering check (the expansion is
                  strictly ascending, or the call is refused) that leaves no room for a wrong, missing or repeated hash.
k_unpack_csr      packed databases small enough to be looked at -- sketches of 0, 1, 2, 255..257, 511..513 hashes, empty ones
                  first, last and in runs, widths 0..64 -- forced through the chunked device expansion in a child process
                  (tuning variables are read once per process) under four chunk plans, against the oracle on the plain arrays
                  and against the host unpack of the same blob.
k_compact_rows    N around 32, 64, 2048 and 4096, hit patterns that fill and empty whole mask words and workgroups, capacities
                  at and below the row count, canaries behind the rows.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import packed_cases as pc
from oracle import oracle
from yacht_amd import _lib
from yacht_amd.engine import ROW_DTYPE, YH_DB_DEFAULT, YH_DB_PAIRWISE_ONLY, PinnedArray, RefDB, csr_pack, pack_sample

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A5A5A5A


def _csr(refs):
    offsets = np.zeros(len(refs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in refs], dtype=np.uint64)
    values = np.concatenate([np.asarray(r, dtype=np.uint64) for r in refs]) if int(offsets[-1]) else np.zeros(0, np.uint64)
    return np.ascontiguousarray(values), offsets


def _want_rows(values, offsets, sample):
    ov = oracle.overlap(values, offsets, sample)
    e, m = oracle.exclusive(values, offsets, ov > 0, sample)
    keep = np.flatnonzero(ov)
    want = np.zeros(keep.size, dtype=ROW_DTYPE)
    want["ref"], want["overlap"], want["n_excl"], want["n_match"] = keep, ov[keep], e[keep], m[keep]
    return want


def _u32(rows):
    return np.ascontiguousarray(rows).view(np.uint32).reshape(-1, 4)


def _assert_rows(got, want, label):
    assert got.size == want.size, (label, got.size, want.size)
    g, w = _u32(got), _u32(want)
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).any(axis=1))
        raise AssertionError(f"{label}: {bad.size} of {want.size} rows differ, first at {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}")


# ---- k_unpack_sample ---------------------------------------------------------------------------------------------------
def _observers(s):
    """The references that see every hash of sample s: s whole, its 256-hash blocks, its hashes by the bits of their lane."""
    lane = np.arange(s.size) % pc.BLOCK
    return [s] + [s[b: b + pc.BLOCK] for b in range(0, s.size, pc.BLOCK)] + [s[(lane >> t) & 1 == 1] for t in range(8)]


@functools.lru_cache(maxsize=1)
def _sample_groups():
    cases = pc.sample_cases()
    full = [c for c in cases if c.name.startswith("full")]
    tails = [c for c in cases if c.name.startswith("n")]
    edges = [c for c in cases if c not in full and c not in tails]
    groups = {f"full_{k}": full[k::4] for k in range(4)}
    groups["tails"] = tails
    groups["edges"] = edges
    assert all(groups.values())
    return groups


@pytest.mark.parametrize("group", ["full_0", "full_1", "full_2", "full_3", "tails", "edges"])
def test_unpack_sample_every_hash_observed(hip_lib, group):
    cases = _sample_groups()[group]
    refs, own = [], []
    for c in cases:
        obs = _observers(c.hashes)
        own.append((len(refs), len(refs) + len(obs)))
        refs += obs
    values, offsets = _csr(refs)
    sizes = np.diff(offsets).astype(np.uint32)
    n_refs = len(refs)
    with RefDB(values, offsets) as db:
        for c, (r0, r1) in zip(cases, own):
            s = c.hashes
            want = _want_rows(values, offsets, s)
            dense = np.zeros(n_refs, dtype=np.uint32)
            dense[want["ref"]] = want["overlap"]
            assert np.array_equal(dense[r0:r1], sizes[r0:r1]), c.name      # (the oracle on its own sample: every observer is full)
            got = db.run_rows(s, packed=True)
            dense = np.zeros(n_refs, dtype=np.uint32)
            dense[got["ref"]] = got["overlap"]
            short = np.flatnonzero(dense[r0:r1] != sizes[r0:r1])
            assert short.size == 0, (c.name, c.widths, "observers (0: whole, then blocks, the last 8: lane bits) that miss hashes",
                                     [(int(k), int(dense[r0 + k]), int(sizes[r0 + k])) for k in short[:12]])
            _assert_rows(got, want, f"{c.name} packed")
            _assert_rows(db.run_rows(s, packed=False), want, f"{c.name} raw")


@pytest.mark.parametrize("pinned", [True, False])
def test_unpack_sample_through_every_slot(hip_lib, pinned):
    """The submit form over all slots, two rounds and more per slot, the packed bytes and the rows in page-locked or in
    pageable memory: cuts of one large case (a cut moves every hash to another lane and changes the widths), observed by
    the database made of the uncut one."""
    a = max(_sample_groups()["full_1"] + _sample_groups()["full_0"], key=lambda c: len(c.h)).hashes
    assert a.size > 4 * pc.BLOCK
    variants = [a, a[1:], a[255:], a[257:-1], a[::2], a[1::3], a[:1], a[:0], a[63: 63 + 2 * pc.BLOCK + 1]]
    values, offsets = _csr(_observers(a))
    want = [_want_rows(values, offsets, v) for v in variants]
    for v, w in zip(variants, want):
        assert v.size == 0 or (w["ref"][0] == 0 and w["overlap"][0] == v.size)
    keep = []

    def buf(k, dt):
        if pinned:
            pa = PinnedArray(k, dt)
            keep.append(pa)
            return pa.array
        return np.zeros(k, dt)

    n_refs = offsets.size - 1
    with RefDB(values, offsets) as db:
        depth = _lib.YH_RUN_SLOTS
        rows = [buf(n_refs, ROW_DTYPE) for _ in range(depth)]
        held = [None] * depth
        order = list(range(len(variants))) * 2
        assert len(order) >= 2 * depth
        for i, vi in enumerate(order + [None] * depth):
            slot = i % depth
            if i >= depth:
                k = db.run_wait_rows(slot)
                _assert_rows(rows[slot][:k], want[order[i - depth]], f"call {i - depth} in slot {slot}")
            if vi is not None:
                p = pack_sample(variants[vi])
                h = buf(p.size, np.uint8)
                h[:] = p
                held[slot] = h
                db.run_submit_packed(slot, h, rows[slot])
    for pa in keep:
        pa.close()


def test_forged_orderings_are_refused_by_the_expansion(hip_lib):
    """Two ordering errors the format cannot exclude and the existing forgeries do not reach: a base that makes only the LAST
    lane of a full block pass 2^64 (seen by the fourth wave alone), and a block whose last hash EQUALS the next block's
    base.  Both are well-formed otherwise (tests/test_packed_cases_cpu.py); both come back as YH_ERR_UNSORTED at wait, the
    good sample queued between them is answered, and so is the handle afterwards."""
    good1, wraps = pc.forge_last_lane_wraps(pack_sample)
    good2, meets = pc.forge_block_meets_next_base(pack_sample)
    values, offsets = _csr(_observers(good2) + _observers(good1))
    want1, want2 = _want_rows(values, offsets, good1), _want_rows(values, offsets, good2)
    n_refs = offsets.size - 1
    with RefDB(values, offsets) as db:
        rows = [np.zeros(n_refs, dtype=ROW_DTYPE) for _ in range(3)]
        db.run_submit_packed(1, wraps, rows[0])
        db.run_submit_packed(2, pack_sample(good2), rows[1])
        db.run_submit_packed(3, meets, rows[2])
        with pytest.raises(_lib.YachtHipError) as ei:
            db.run_wait_rows(1)
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        _assert_rows(rows[1][: db.run_wait_rows(2)], want2, "the good sample between the forged ones")
        with pytest.raises(_lib.YachtHipError) as ei:
            db.run_wait_rows(3)
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        _assert_rows(db.run_rows(good1), want1, "afterwards")
        _assert_rows(db.run_rows(good2, packed=False), want2, "afterwards, raw")


# ---- k_unpack_csr ------------------------------------------------------------------------------------------------------
def csr_report():
    """Every database of packed_cases.csr_database created from its packed form, as a train handle and as a full handle,
    against the oracle on the plain arrays.  Called in the child processes (device expansion) and in the test process (host
    unpack); the digests make "the same results" comparable across the two."""
    out = {}
    for kind in pc.CSR_KINDS:
        values, offsets, _ = pc.csr_database(kind)
        blob = csr_pack(values, offsets)
        sizes = np.diff(offsets).astype(np.uint32)
        sample = np.unique(values)
        want_ov = oracle.overlap(values, offsets, sample)
        want_e, want_m = oracle.exclusive(values, offsets, want_ov > 0, sample)
        want_pairs = {c: oracle.train_pairs(values, offsets, c, threads=4) for c in (0.0, 0.3)}
        for flags in (YH_DB_PAIRWISE_ONLY, YH_DB_DEFAULT):
            rep, dig = {}, hashlib.sha256()
            with RefDB.from_packed(blob, flags=flags) as db:
                for c, (wi, wj, wc, wstats) in want_pairs.items():
                    gi, gj, gc = db.pairwise(c)
                    rep[f"pairs_{c}_ok"] = bool(np.array_equal(gi, wi) and np.array_equal(gj, wj) and np.array_equal(gc, wc))
                    rep[f"n_pairs_{c}"] = int(gi.size)
                    for a in (gi, gj, gc):
                        dig.update(np.ascontiguousarray(a).tobytes())
                stats = tuple(int(x) for x in db.index_stats())
                rep["stats"] = list(stats)
                rep["stats_ok"] = stats == tuple(int(x) for x in want_pairs[0.0][3])
                rep["n_distinct_ok"] = stats[0] == int(sample.size)
                rep["n_hashes_ok"] = int(db.info()["n_hashes"]) == int(values.size)
                if flags == YH_DB_DEFAULT:
                    ov, e, m = db.run_counts(sample)
                    rep["covers_ok"] = bool(np.array_equal(ov, sizes))
                    rep["run_ok"] = bool(np.array_equal(ov, want_ov) and np.array_equal(e, want_e) and np.array_equal(m, want_m))
                    for a in (ov, e, m):
                        dig.update(np.ascontiguousarray(a).tobytes())
            rep["digest"] = dig.hexdigest()
            out[f"{kind}_flags{flags}"] = rep
    return out


CSR_WORKER = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_packed_edges as t
print(json.dumps(t.csr_report()))
"""


@pytest.fixture(scope="module")
def host_unpack_report(hip_lib):
    """The same blobs in this process, which has no tuning variables: databases this small are unpacked on the host."""
    return csr_report()


def _assert_report(rep, label):
    assert len(rep) == 2 * len(pc.CSR_KINDS)
    for key, r in rep.items():
        oks = {k: v for k, v in r.items() if k.endswith("_ok")}
        assert len(oks) == (7 if key.endswith(f"flags{YH_DB_DEFAULT}") else 5), (label, key, r)
        assert all(oks.values()), (label, key, r)
    assert rep[f"sizes_flags{YH_DB_DEFAULT}"]["n_pairs_0.3"] > 4 and rep[f"tiny_flags{YH_DB_DEFAULT}"]["n_pairs_0.0"] > 100   # (pairs there are)


def test_packed_csr_small_databases_through_the_host_unpack(hip_lib, host_unpack_report):
    _assert_report(host_unpack_report, "host unpack")


@pytest.mark.parametrize("shares", [None, "0.5,0.5", "0.05,0.05,0.9", "0.25,0.25,0.25,0.125,0.125"])
def test_unpack_csr_on_device(hip_lib, host_unpack_report, shares):
    """yh_db_create_packed forced onto the chunked upload (YH_UPLOAD_CHUNK_MIN=1): k_unpack_csr expands every chunk's
    blocks; the chunk plans put their cuts next to the empty sketches and inside the run of tiny ones.  The trace line
    of the packed branch proves which expansion ran."""
    env = dict(os.environ)
    env.update({"YH_DEBUG_TUNING": "1", "YH_UPLOAD_CHUNK_MIN": "1", "YH_CHECK_SORT": "1", "YH_TRACE_BUILD": "1"})
    env.pop("YH_UPLOAD_SHARES", None)
    if shares:
        env["YH_UPLOAD_SHARES"] = shares
    r = subprocess.run([sys.executable, "-c", CSR_WORKER, ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    _assert_report(out, f"device expansion, shares {shares}")
    assert out == host_unpack_report
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[yh build] packed chunk ") and ln.endswith("expanded on the device")]
    firsts = [ln for ln in lines if " packed chunk 1 of " in ln]
    assert len(firsts) == 2 * len(pc.CSR_KINDS), r.stderr[-2000:]      # every create went through the device expansion
    plans = [int(ln.split(" of ")[1].split(":")[0]) for ln in firsts]
    assert len(lines) == sum(plans)
    assert max(plans) == (4 if shares is None else len(shares.split(","))), plans   # (every cut of the plan was made somewhere)
    assert min(plans) >= 2


# ---- k_compact_rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.ROWS_N)
def test_compact_rows_at_their_boundaries(hip_lib, n):
    import torch

    values, offsets = pc.rows_database(n)
    with RefDB(values, offsets) as db:
        for name, hit in pc.rows_patterns(n).items():
            label = f"N={n} {name}"
            s = pc.rows_sample(n, hit)
            want = _want_rows(values, offsets, s)
            assert np.array_equal(want["ref"], hit), label
            k = want.size
            # host form, both uploads (4 097 rows: the first buffer is too small, the second holds exactly the rows)
            _assert_rows(db.run_rows(s, packed=True), want, label + " packed")
            _assert_rows(db.run_rows(s, packed=False), want, label + " raw")
            # device form: the step, then its rows into buffers of several capacities with canaries behind them
            d_s = torch.from_numpy(s.view(np.int64).copy()).cuda()
            c = torch.zeros(3, n, dtype=torch.int32, device="cuda")
            db.run_device(d_s.data_ptr(), d_s.numel(), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr())
            for cap in ([k, k - 1, 1] if k >= 2 else [k]):
                rows = torch.full((cap + 8, 4), CANARY, dtype=torch.int32, device="cuda")
                cnt = torch.full((1,), CANARY, dtype=torch.int32, device="cuda")
                db.run_rows_device(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), rows.data_ptr(), cap, cnt.data_ptr())
                db.synchronize()
                got = rows.cpu().numpy().view(np.uint32)
                assert int(cnt.item()) == k, (label, cap, int(cnt.item()), k)
                assert np.array_equal(got[:cap], _u32(want)[:cap]), (label, cap)
                assert (got[cap:] == CANARY).all(), (label, cap, "rows behind the capacity were written")
            if k < 2:
                continue
            # host form with room for one row less: YH_ERR_CAPACITY, the number needed, a valid prefix, nothing behind it
            cap = k - 1
            pin = PinnedArray(cap + 8, ROW_DTYPE)
            page = np.zeros(cap + 8, dtype=ROW_DTYPE)
            for slot, buf, packed in ((1, pin.array, True), (2, page, False)):
                _u32(buf)[:] = CANARY
                if packed:
                    p = pack_sample(s)
                    db.run_submit_packed(slot, p, buf[:cap])
                else:
                    db.run_submit_rows(slot, s, buf[:cap])
                need = C.c_uint64(0)
                rc = db._lib.yh_run_wait_rows(db._h, slot, C.byref(need))
                assert rc == _lib.YH_ERR_CAPACITY and int(need.value) == k, (label, slot, rc, int(need.value), k)
                assert np.array_equal(_u32(buf)[:cap], _u32(want)[:cap]), (label, slot)
                assert (_u32(buf)[cap:] == CANARY).all(), (label, slot)
            pin.close()
