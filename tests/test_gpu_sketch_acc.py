"""The sketch accumulator (yh_sketch_acc_* in yacht_amd/csrc/yh_sketch.hip): one sketch with abundances out of many chunks.
Every comparison is exact -- array_equal on the hashes and on the counts -- against a collections.Counter over
tests/sketch_scalar.kmer_hashes (the larger input: against oracle/sketch_oracle.py).  The contract under test is chunking
invariance: the result depends on the multiset of kept hashes alone, not on the chunks, the log's capacity or the moments of
compaction."""
import collections
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import sketch_scalar as ss
from oracle import sketch_oracle as so

pytestmark = pytest.mark.gpu

FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")
M64 = 2 ** 64 - 1
CAPS = [1, 255, 256, 257, 0]          # cap_entries: around one workgroup of the compaction kernels (256 lanes), and the default
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _reads():
    """42 reads of 100..150 bases: 36 random ones, three of them again, and three as reverse complements (counts above 1)"""
    rng = np.random.default_rng(20240607)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(n)).tobytes()) for n in rng.integers(100, 151, size=36)]
    reads[5] = reads[5][:60] + b"N" + reads[5][61:]      # a byte that is not a base breaks the windows over it
    reads[6] = reads[6].lower()
    return reads + [reads[0], reads[7], reads[20]] + [r.translate(_COMP)[::-1] for r in (reads[1], reads[7], reads[30])]


READS = _reads()
_hash_cache = {}


def hashes_of(read, k):
    key = (read, k)
    if key not in _hash_cache:
        _hash_cache[key] = ss.kmer_hashes(read, k)
    return _hash_cache[key]


def counter_of(reads, k, max_hash):
    c = collections.Counter()
    for r in reads:
        c.update(h for h in hashes_of(r, k) if h <= max_hash)
    return c


def arrays_of(counter):
    keys = sorted(counter)
    return np.array(keys, dtype=np.uint64), np.array([counter[h] for h in keys], dtype=np.uint64)


def chunkings(reads):
    uneven, at = [], 0
    for n in (1, 7, 2, 13, 1, 5, len(reads)):
        if at < len(reads):
            uneven.append(b"\n".join(reads[at:at + n]))
            at += n
    return {"one": [b"\n".join(reads)], "per-read": list(reads), "uneven": uneven}


def acc_result(chunks, k, scaled, cap_entries=0):
    from yacht_amd import sketch

    with sketch.SketchAccumulator(k, scaled, cap_entries=cap_entries) as acc:
        for c in chunks:
            acc.add(c)
        mins, counts = acc.finish()
        return mins, counts, acc.info()


def _same(got, want):
    return got[0].dtype == np.uint64 and got[1].dtype == np.uint64 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [1, 10])
@pytest.mark.parametrize("k", [21, 31])
def test_result_does_not_depend_on_chunks_or_capacity(hip_lib, k, scaled):
    mh = so.max_hash_for_scaled(scaled)
    want = arrays_of(counter_of(READS, k, mh))
    assert want[0].size > (300 if scaled == 10 else 3000) and int(want[1].max()) >= 2
    kept_total = int(want[1].sum())
    kept_first = {name: sum(1 for h in ss.kmer_hashes(cs[0], k) if h <= mh) for name, cs in chunkings(READS).items()}
    for name, chunks in chunkings(READS).items():
        for cap in CAPS:
            mins, counts, info = acc_result(chunks, k, scaled, cap)
            assert _same((mins, counts), want), (name, cap)
            assert info["n_kept"] == kept_total and info["n_bytes"] == sum(len(c) for c in chunks), (name, cap, info)
            assert info["n_entries"] == info["n_compacted"] == want[0].size <= info["capacity"], (name, cap, info)
            if cap == 1:
                assert info["n_compactions"] >= 1, (name, info)
            if cap and kept_first[name] > cap:     # the first chunk keeps more than the empty log holds
                assert info["n_rehashed_chunks"] >= 1, (name, cap, info)
            if cap == 0:
                assert info["n_rehashed_chunks"] == 0 and info["n_compactions"] == 1 and info["capacity"] == 1 << 21, (name, info)


def test_duplicates_across_chunks(hip_lib):
    k, read = 31, READS[3]
    single = counter_of([read], k, M64)
    rc = read.translate(_COMP)[::-1]
    mins, counts, _ = acc_result([read, read, read, rc], k, 1, cap_entries=64)
    want = arrays_of(collections.Counter({h: 4 * c for h, c in single.items()}))
    assert _same((mins, counts), want)


def test_one_long_run_counts_past_65535(hip_lib):
    k = 31
    poly = b"A" * 70030
    (h_poly,) = set(ss.kmer_hashes(poly[:40], k))
    for cap in (0, 1000):
        mins, counts, _ = acc_result([poly], k, 1, cap)
        assert mins.tolist() == [h_poly] and counts.tolist() == [70000], cap
        mins, counts, _ = acc_result([poly, poly], k, 1, cap)
        assert mins.tolist() == [h_poly] and counts.tolist() == [140000], cap
    others = counter_of(READS, k, M64)
    assert h_poly not in others
    mixed = collections.Counter(others)
    mixed[h_poly] = 140000
    half = len(READS) // 2
    chunks = [b"\n".join(READS[:half]), poly, b"\n".join(READS[half:]) + b"\n" + poly]
    for cap in (0, 300):
        mins, counts, _ = acc_result(chunks, k, 1, cap)
        assert _same((mins, counts), arrays_of(mixed)), cap


# ---- edges through add_hashes ----------------------------------------------------------------------------------------------
def _acc(max_hash, cap_entries=0, k=31):
    from yacht_amd import sketch

    return sketch.SketchAccumulator(k, max_hash=max_hash, cap_entries=cap_entries)


def test_add_hashes_edges(hip_lib):
    from yacht_amd import _lib

    mh = so.max_hash_for_scaled(1000)
    with _acc(mh, cap_entries=4) as acc:
        acc.add_hashes([mh, 0, 5, 0])
        acc.add_hashes([], [])                                   # n = 0
        acc.add_hashes(np.zeros(0, np.uint64))
        acc.add_hashes([5, mh, 7], [2 ** 32 + 5, 3, 2 ** 33])
        acc.add_hashes([5, 5], [2 ** 32 + 5, 2 ** 32 + 5])       # 3 * 2^32 + 15 > 2^33
        before = acc.info()
        with pytest.raises(_lib.YachtHipError) as ei:            # one hash above max_hash: refused, nothing added
            acc.add_hashes([1, mh + 1, 2])
        assert ei.value.code == _lib.YH_ERR_INVALID_ARG and "max_hash" in str(ei.value)
        assert acc.info() == before
        mins, counts = acc.finish()
        assert mins.tolist() == [0, 5, 7, mh] and counts.tolist() == [2, 1 + 3 * (2 ** 32 + 5), 2 ** 33, 4]
        assert int(counts[1]) > 2 ** 33
    with _acc(M64, cap_entries=2) as acc:                        # every bit of the key is sorted on
        acc.add_hashes([M64, 0, M64 - 1, M64, 1 << 63])
        mins, counts = acc.finish()
        assert mins.tolist() == [0, 1 << 63, M64 - 1, M64] and counts.tolist() == [1, 1, 1, 2]
    with _acc(0) as acc:
        acc.add_hashes([0, 0, 0])
        with pytest.raises(_lib.YachtHipError):
            acc.add_hashes([1])
        assert [x.tolist() for x in acc.finish()] == [[0], [3]]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_add_hashes_around_one_workgroup(hip_lib, n):
    rng = np.random.default_rng(n)
    mh = so.max_hash_for_scaled(10)
    distinct = np.unique(rng.integers(0, mh, size=n + 50, dtype=np.uint64))[:n]
    assert distinct.size == n
    again = rng.permutation(distinct)[: n // 3]
    order = rng.permutation(np.concatenate([distinct, again]))
    want = collections.Counter(order.tolist())
    for cap in (1, n, 0):
        with _acc(mh, cap_entries=cap) as acc:
            for part in np.array_split(order, 3):
                acc.add_hashes(part)
            assert _same(acc.finish(), arrays_of(want)), cap
    with _acc(mh, cap_entries=n) as acc:                          # exactly full, sorted, no duplicates: compaction keeps all
        acc.add_hashes(distinct)
        mins, counts = acc.finish()
        assert np.array_equal(mins, distinct) and counts.tolist() == [1] * n
        assert acc.info()["capacity"] == 2 * n                   # as many entries free as distinct ones


# ---- lifecycle -------------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime the process already uses (the copy yacht_amd._lib loads first: torch's, when torch is installed)"""
    spec = importlib.util.find_spec("torch")
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else ""
    return C.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")


def _device_words(ptr, n):
    out = np.empty(n, dtype=np.uint64)
    if n:
        hip = _hip_runtime()
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), 8 * n, 2) == 0   # hipMemcpyDeviceToHost
    return out


def test_lifecycle(hip_lib):
    from yacht_amd import _lib, sketch

    k, scaled = 21, 10
    mh = so.max_hash_for_scaled(scaled)
    first, second = READS[:10], READS[10:25]
    with sketch.SketchAccumulator(k, scaled, cap_entries=100) as acc:
        assert [x.size for x in acc.finish()] == [0, 0]           # empty
        acc.add(b"ACGTACGTACGTACGTACGT")                          # shorter than k: nothing
        acc.add(b"")
        assert [x.size for x in acc.finish()] == [0, 0] and acc.info()["n_kept"] == 0 and acc.info()["n_bytes"] == 20
        acc.add(b"\n".join(first))
        want1 = arrays_of(counter_of(first, k, mh))
        assert _same(acc.finish(), want1)
        assert _same(acc.finish(), want1)                         # (again: the same)
        acc.add(b"\n".join(second))                               # finish does not end the accumulator
        want2 = arrays_of(counter_of(first + second, k, mh))
        # two-call sizing by hand: count, too small, exact
        n = C.c_uint64(0)
        lib, h = hip_lib, acc._h
        assert lib.yh_sketch_acc_finish(h, 0, None, None, C.byref(n)) == _lib.YH_OK and n.value == want2[0].size
        small = want2[0].size - 1
        m = np.full(want2[0].size + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        a = m.copy()
        n = C.c_uint64(0)
        assert lib.yh_sketch_acc_finish(h, small, C.c_void_p(m.ctypes.data), C.c_void_p(a.ctypes.data), C.byref(n)) == _lib.YH_ERR_CAPACITY
        assert n.value == want2[0].size and b"needed" in lib.yh_last_error()
        assert lib.yh_sketch_acc_finish(h, n.value, C.c_void_p(m.ctypes.data), C.c_void_p(a.ctypes.data), C.byref(n)) == _lib.YH_OK
        assert _same((m[:n.value], a[:n.value]), want2) and bool(np.all(m[n.value:] == np.uint64(0xA5A5A5A5A5A5A5A5)))
        assert bool(np.all(a[n.value:] == np.uint64(0xA5A5A5A5A5A5A5A5)))
        # the device form: pointers into the state
        d_m, d_a, nd = acc.finish_device()
        assert nd == want2[0].size and _same((_device_words(d_m, nd), _device_words(d_a, nd)), want2)
        assert lib.yh_sketch_acc_finish(h, 4, None, None, C.byref(n)) == _lib.YH_ERR_INVALID_ARG
    with pytest.raises(_lib.YachtHipError):                      # closed
        acc.add(b"A" * 40)


def test_add_device_equals_add(hip_lib):
    import torch
    from yacht_amd import sketch

    k, scaled = 31, 10
    chunks = chunkings(READS)["uneven"]
    want = arrays_of(counter_of(READS, k, so.max_hash_for_scaled(scaled)))
    for shift in (0, 3):    # (3: not 16-byte aligned, the byte-wise kernel)
        with sketch.SketchAccumulator(k, scaled, cap_entries=300) as acc:
            for c in chunks:
                d = torch.full((shift + len(c) + 64,), ord("A"), dtype=torch.uint8, device="cuda")
                d[shift:shift + len(c)] = torch.from_numpy(np.frombuffer(c, dtype=np.uint8).copy())
                torch.cuda.synchronize()
                acc.add_device(d.data_ptr() + shift, len(c))
            assert _same(acc.finish(), want), shift


def test_bad_arguments(hip_lib):
    from yacht_amd import _lib

    h = C.c_void_p()
    assert hip_lib.yh_sketch_acc_create(1 << 20, 31, 42, M64, 0, C.byref(h)) == _lib.YH_ERR_NO_DEVICE and not h
    assert hip_lib.yh_sketch_acc_create(-1, 31, 42, M64, 0, C.byref(h)) == _lib.YH_ERR_NO_DEVICE and not h
    assert b"out of range" in hip_lib.yh_last_error()
    assert hip_lib.yh_sketch_acc_create(0, 31, 42, M64, 8, C.byref(h)) == _lib.YH_OK and h
    assert hip_lib.yh_sketch_acc_add(h, None, 40) == _lib.YH_ERR_INVALID_ARG
    assert hip_lib.yh_sketch_acc_add_hashes(h, None, None, 3) == _lib.YH_ERR_INVALID_ARG
    assert hip_lib.yh_sketch_acc_get_info(h, None) == _lib.YH_ERR_INVALID_ARG
    assert hip_lib.yh_sketch_acc_destroy(h) == _lib.YH_OK


# ---- larger input ----------------------------------------------------------------------------------------------------------
def test_genome_reads_in_64k_chunks(hip_lib):
    from yacht_amd import sketch

    seq = b"".join(s for _n, s in so.read_fasta(os.path.join(FX, "GCF_018918045.1_genomic.fna.gz")))[:2_000_000]
    reads = [seq[i:i + 150] for i in range(0, len(seq), 150)]
    reads += reads[::10]                                         # every tenth read twice
    want_m, want_a = so.sketch_records(reads, 31, 1000)
    assert want_m.size > 1000 and int(np.max(want_a)) >= 2
    chunks, batch, held = [], [], 0
    for r in reads:
        if batch and held + 1 + len(r) > 65536:
            chunks.append(b"\n".join(batch))
            batch, held = [], 0
        held += len(r) + (1 if batch else 0)
        batch.append(r)
    chunks.append(b"\n".join(batch))
    assert len(chunks) > 30 and max(len(c) for c in chunks) <= 65536
    ref_m, ref_a = sketch.sketch_sequences(reads, 31, 1000)
    assert np.array_equal(ref_m, want_m) and np.array_equal(ref_a, want_a)
    for cap in (0, 512):
        mins, counts, info = acc_result(chunks, 31, 1000, cap)
        assert np.array_equal(mins, ref_m) and np.array_equal(counts.astype(np.int64), ref_a), cap
        assert info["n_kept"] == int(want_a.sum())
    assert info["n_compactions"] >= 2
