"""The sketch kernels of yacht_amd/csrc/yh_sketch.hip at their edges, against oracle/sketch_oracle.py (which
tests/test_sketch_oracle_pins.py pins from outside).  Every comparison is exact: equal uint64 multisets (sort and
array_equal) or equal counts.  The shapes are the smallest at which each mechanism of the kernels exists.

The case builders at the top need no GPU; tests/test_sketch_oracle_pins.py imports them."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import sketch_oracle as so

# the geometry of yh_sketch.hip, by its names there
UNIT = 16              # bases per staged unit (one 16-byte load, one lcode/lbad word)
RL_RUN = 32            # windows per lane of the 2-bit kernels
RL_WIN = 8192          # windows per workgroup of the 2-bit kernels (RL_THREADS * RL_RUN)
SK_WIN = 2048          # windows per workgroup of the byte-wise kernel (SK_THREADS * SK_ITEMS)
SK_LCAP = 2048         # kept hashes a workgroup parks in LDS before they overflow to global memory

FULL = 2 ** 64 - 1
PREFILL = 0xA5A5A5A5A5A5A5A5
CANARY = 64
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_ACGTacgt = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


# ---- case builders (CPU only) ------------------------------------------------------------------------------------------------
def _u8(seq):
    return np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)


def kernel_of(k, shift):
    """which kernel launch_sketch picks: '64' / '128' (2-bit kernel on a 64- / 128-bit word) or 'bytes'"""
    if k > 64 or shift % 16:
        return "bytes"
    return "64" if k <= 32 else "128"


def valid_windows(seq_u8, k):
    """bool per window: made of A/C/G/T (either case) only.  Its own statement (a running count of other bytes)."""
    s = _u8(seq_u8)
    if s.size < k:
        return np.zeros(0, dtype=bool)
    bad = np.concatenate(([0], np.cumsum(~np.isin(s, _ACGTacgt))))
    return (bad[k:] - bad[:-k]) == 0


def oracle_hashes(seq_u8, k, seed=42, max_hash=FULL):
    h = so.kmer_hashes(_u8(seq_u8).tobytes(), k, seed)
    return np.sort(h[h <= np.uint64(max_hash)])


def without_windows(H, k, positions):
    """sorted hashes of an all-valid sequence (H in window order) after a bad base at each of `positions`: the windows
    [p - k + 1, p] go."""
    keep = np.ones(H.size, dtype=bool)
    for p in positions:
        keep[max(0, p - k + 1):p + 1] = False
    return np.sort(H[keep])


def low_complexity(k, extra=RL_WIN + 100):
    """T5: name -> sequence of length k + extra (every one has a period of at most 4)"""
    n = k + extra
    return {name: (unit * (n // len(unit) + 1))[:n] for name, unit in
            (("polyA", b"A"), ("polyT", b"T"), ("AT", b"AT"), ("CG", b"CG"), ("ACGT", b"ACGT"))}


def palindrome_family(k):
    """T5: P = H + revcomp(H) (its own reverse complement) and all 3k single substitutions of it, joined by N"""
    assert k % 2 == 0
    rng = np.random.default_rng(1000 + k)
    h = _ACGT[rng.integers(0, 4, size=k // 2)].tobytes()
    p = h + h.translate(_COMP)[::-1]
    assert p.translate(_COMP)[::-1] == p
    out = [p]
    for i in range(k):
        out += [p[:i] + bytes([b]) + p[i + 1:] for b in b"ACGT" if b != p[i]]
    assert len(out) == 3 * k + 1
    return b"N".join(out)


FUZZ_KS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 21, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 127, 255)
FUZZ_CASES = 300
FUZZ_SEED = 20240607


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    """T8: the 300 cases, as dicts k, n, density, shift, scaled, seed, seq (read-only uint8).  k, density, scaled and seed
    are drawn as the list above says.  Two weights make the rare classes occur at all: 6 % of the cases draw n below k
    and 8 % draw n in [k, k + 8) with a density of 1/k or 3/k (few windows, most of them broken), the rest draw n
    uniformly below 3 * 8192; and half of the cases are aligned (shift 0), the other half draw shift from 0..15,
    because only an aligned pointer reaches the 2-bit kernels.  tests/test_sketch_oracle_pins.py asserts what the list
    must cover."""
    rng = np.random.default_rng(FUZZ_SEED)
    cases = []
    for _ in range(FUZZ_CASES):
        k = int(rng.choice(FUZZ_KS))
        density = float(rng.choice((0.0, 0.2 / k, 1.0 / k, 3.0 / k)))
        n = int(rng.integers(0, 3 * RL_WIN))
        u = rng.random()
        if u < 0.06:
            n = int(rng.integers(0, k))
        elif u < 0.14:
            n = k + int(rng.integers(0, 8))
            density = float(rng.choice((1.0 / k, 3.0 / k)))
        shift = int(rng.integers(0, 16))
        if rng.random() < 0.5:
            shift = 0
        scaled = int(rng.choice((1, 3, 50)))
        seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        seq = _ACGTacgt[rng.integers(0, 8, size=n)]
        bad = rng.random(n) < density
        seq[bad] = rng.integers(0, 256, size=int(bad.sum()), dtype=np.uint8)
        seq.setflags(write=False)
        cases.append(dict(k=k, n=n, density=density, shift=shift, scaled=scaled, seed=seed, seq=seq))
    return tuple(cases)


def fuzz_expected(case):
    """the kept hashes of a fuzz case in window order, and the window each came from"""
    h = so.kmer_hashes(case["seq"].tobytes(), case["k"], case["seed"])
    win = np.flatnonzero(valid_windows(case["seq"], case["k"]))
    assert win.size == h.size
    keep = h <= np.uint64(so.max_hash_for_scaled(case["scaled"]))
    return h[keep], win[keep]


@functools.lru_cache(maxsize=None)
def random_bases(n, seed, lower=False):
    rng = np.random.default_rng(seed)
    seq = (_ACGTacgt[rng.integers(0, 8, size=n)] if lower else _ACGT[rng.integers(0, 4, size=n)]).copy()
    seq.setflags(write=False)
    return seq


@functools.lru_cache(maxsize=None)
def base_hashes(n, seed, k, lower=False):
    """hashes of random_bases(n, seed) in window order (all windows are valid: one per window)"""
    h = so.kmer_hashes(random_bases(n, seed, lower).tobytes(), k)
    assert h.size == n - k + 1
    h.setflags(write=False)
    return h


# ---- the device helper -------------------------------------------------------------------------------------------------------
def dev_sketch(seq_u8, k, seed=42, max_hash=FULL, cap=None, shift=0, expect_rc=0):
    """yh_sketch_dna_device on the sequence placed `shift` bytes into a fresh 16-byte aligned device buffer (the bytes
    around it are 'A': valid bases, so a read outside the sequence shows as extra hashes).  cap None = one slot per
    window.  -> (count, the cap output words, the 64 words behind them); an output word nobody wrote holds PREFILL.
    cap 0 passes a null output pointer, n 0 a null sequence pointer."""
    import torch

    from yacht_amd import _lib

    lib = _lib.load()
    seq = _u8(seq_u8)
    n = int(seq.size)
    if cap is None:
        cap = max(n - k + 1, 0)
    buf = torch.full((shift + n + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if n:
        buf[shift:shift + n] = torch.from_numpy(np.array(seq))
    d_seq = buf[shift:]
    # (what makes "this case ran the 2-bit / the byte-wise kernel" true: launch_sketch decides by this)
    assert d_seq.data_ptr() % 16 == shift % 16
    out = torch.full((cap + CANARY,), PREFILL - 2 ** 64, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    rc = lib.yh_sketch_dna_device(C.c_void_p(d_seq.data_ptr()) if n else None, n, k, seed, max_hash, cap,
                                  C.c_void_p(out.data_ptr()) if cap else None, C.c_void_p(cnt.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.yh_last_error())
    host = out.cpu().numpy().view(np.uint64)
    return int(cnt.item()), host[:cap], host[cap:]


def check_against(want_sorted, seq_u8, k, what, **kw):
    """one launch with room for every window: exactly the wanted multiset, nothing behind it"""
    count, stored, canary = dev_sketch(seq_u8, k, **kw)
    assert count == want_sorted.size, (what, count, want_sorted.size)
    assert np.array_equal(np.sort(stored[:count]), want_sorted), what
    assert bool(np.all(stored[count:] == np.uint64(PREFILL))) and bool(np.all(canary == np.uint64(PREFILL))), what


def is_submultiset(a, b):
    ua, ca = np.unique(a, return_counts=True)
    ub, cb = np.unique(b, return_counts=True)
    idx = np.searchsorted(ub, ua)
    if bool(np.any(idx >= ub.size)):
        return False
    return bool(np.all(ub[idx] == ua) and np.all(ca <= cb[idx]))


# ---- T1: every k -------------------------------------------------------------------------------------------------------------
T1_N = RL_WIN + 2 * 255 + 37


@functools.lru_cache(maxsize=None)
def t1_sequence():
    rng = np.random.default_rng(101)
    seq = _ACGTacgt[rng.integers(0, 8, size=T1_N)]
    seq[rng.choice(T1_N, size=24, replace=False)] = ord("N")
    seq.setflags(write=False)
    return seq


@pytest.mark.gpu
@pytest.mark.parametrize("k_lo,k_hi", [(1, 64), (65, 128), (129, 192), (193, 255)])
def test_t1_every_k(hip_lib, k_lo, k_hi):
    seq = t1_sequence()
    assert seq.size == 8739
    for k in range(k_lo, k_hi + 1):
        want = oracle_hashes(seq, k)
        assert 0 < want.size < seq.size - k + 1
        check_against(want, seq, k, ("k", k))
        if k <= 64:
            check_against(want, seq, k, ("k", k, "byte-wise"), shift=1)


# ---- T2: all 256 byte values at all 16 offsets in a unit ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def t2_sequence():
    n = 48 * 4096
    seq = random_bases(n, 202).copy()
    for v in range(256):
        for r in range(UNIT):
            p = 48 * (16 * v + r) + r
            assert p % UNIT == r
            seq[p] = v
    seq.setflags(write=False)
    return seq


@pytest.mark.gpu
@pytest.mark.parametrize("k,shift", [(21, 0), (40, 0), (21, 3), (70, 0)])
def test_t2_every_byte_value_at_every_unit_offset(hip_lib, k, shift):
    seq = t2_sequence()
    want = oracle_hashes(seq, k)
    assert 0 < want.size < seq.size - k + 1   # some byte values break windows, some do not
    assert want.size == int(valid_windows(seq, k).sum())
    check_against(want, seq, k, (k, shift), shift=shift)


# ---- T3: where a bad base sits -----------------------------------------------------------------------------------------------
T3_N = 2 * RL_WIN + 5
T3_SEED = 303


def _with_n(base, positions):
    seq = base.copy()
    seq[list(positions)] = ord("N")
    return seq


def _pair_positions(boundary, k):
    """two bad bases d = k - 1 .. k + 2 apart (0, 0, 1, 2 whole windows between them), the first below `boundary`, the
    second at or above it where d allows"""
    out = []
    for d in (k - 1, k, k + 1, k + 2):
        for p1 in {boundary - d, boundary - 1 - d // 2, boundary - 1}:
            out.append((p1, p1 + d))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 64, 65])
def test_t3_bad_base_scan_across_workgroup_and_lane(hip_lib, k):
    base = random_bases(T3_N, T3_SEED)
    H = base_hashes(T3_N, T3_SEED, k)
    check_against(np.sort(H), base, k, (k, "no bad base"))
    for p in range(RL_WIN - k - 34, RL_WIN + 34):
        check_against(without_windows(H, k, [p]), _with_n(base, [p]), k, (k, p))
    lane = RL_WIN // 2 + RL_RUN     # a lane start that is no workgroup start
    for pair in _pair_positions(RL_WIN, k) + _pair_positions(lane, k):
        check_against(without_windows(H, k, pair), _with_n(base, pair), k, (k, pair))
    for p in (0, T3_N - 1, T3_N - k):
        check_against(without_windows(H, k, [p]), _with_n(base, [p]), k, (k, p))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 64])
def test_t3_bad_base_scan_bytewise(hip_lib, k):
    base = random_bases(T3_N, T3_SEED)
    H = base_hashes(T3_N, T3_SEED, k)
    for boundary in (SK_WIN, 2 * SK_WIN):
        for p in range(boundary - k - 34, boundary + 34):
            check_against(without_windows(H, k, [p]), _with_n(base, [p]), k, (k, p), shift=5)
        for pair in _pair_positions(boundary, k):
            check_against(without_windows(H, k, pair), _with_n(base, pair), k, (k, pair), shift=5)
    for p in (0, T3_N - 1, T3_N - k):
        check_against(without_windows(H, k, [p]), _with_n(base, [p]), k, (k, p), shift=5)


# ---- T4: lengths -------------------------------------------------------------------------------------------------------------
T4_NWIN = (1, 2, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193, 16385)
T4_SEED = 404


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 16, 31, 32, 33, 64, 65, 255])
def test_t4_lengths(hip_lib, k):
    longest = max(T4_NWIN) + k - 1
    base = random_bases(longest, T4_SEED, True)
    H = base_hashes(longest, T4_SEED, k, True)
    for shift in (0, 7):
        for n_win in T4_NWIN:
            n = n_win + k - 1
            check_against(np.sort(H[:n_win]), base[:n], k, (k, n_win, shift), shift=shift)
        for n in sorted({0, 1, k - 1}):
            want = np.sort(H[:max(n - k + 1, 0)])
            assert want.size == (1 if (k == 1 and n == 1) else 0)
            check_against(want, base[:n], k, (k, "n", n, shift), shift=shift)   # (YH_OK asserted in dev_sketch)


# ---- T5: low complexity, self-complementary k-mers ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4, 30, 31, 32, 34, 62, 64, 66, 254])
def test_t5_low_complexity(hip_lib, k):
    got = {}
    for name, seq in low_complexity(k).items():
        assert len(seq) == RL_WIN + k + 100
        want = oracle_hashes(seq, k)
        assert want.size == RL_WIN + 101    # every window kept: 8192 through a 2048-entry list in the first workgroup
        count, stored, canary = dev_sketch(seq, k)
        assert count == want.size and np.array_equal(np.sort(stored), want), (k, name)
        assert bool(np.all(canary == np.uint64(PREFILL)))
        got[name] = stored
    a = np.unique(got["polyA"])
    assert a.size == 1 and got["polyA"].size == RL_WIN + 101
    assert int(a[0]) == int(so.kmer_hashes(b"A" * k, k)[0])
    assert np.array_equal(np.unique(got["polyT"]), a) and got["polyT"].size == RL_WIN + 101


@pytest.mark.gpu
@pytest.mark.parametrize("k", [32, 64, 66])
def test_t5_palindromes_and_their_neighbours(hip_lib, k):
    seq = palindrome_family(k)
    want = oracle_hashes(seq, k)
    assert want.size == 3 * k + 1
    check_against(want, seq, k, k)


# ---- T6: the cap contract ----------------------------------------------------------------------------------------------------
T6_N = 3 * RL_WIN + 30
T6_SEED = 606


def _check_cap(seq, k, max_hash, want_sorted, cap):
    T = want_sorted.size
    count, stored, canary = dev_sketch(seq, k, max_hash=max_hash, cap=cap)
    assert count == T, (cap, count, T)
    m = min(cap, T)
    assert is_submultiset(stored[:m], want_sorted), cap     # (PREFILL is no expected hash: an unwritten slot fails here)
    assert bool(np.all(stored[m:] == np.uint64(PREFILL))), cap
    assert bool(np.all(canary == np.uint64(PREFILL))), cap


@pytest.mark.gpu
def test_t6_cap_device(hip_lib):
    k = 31
    seq = random_bases(T6_N, T6_SEED)
    want = np.sort(base_hashes(T6_N, T6_SEED, k))
    T = want.size
    assert T == 3 * RL_WIN and np.uint64(PREFILL) not in want
    for cap in (0, 1, SK_LCAP - 1, SK_LCAP, SK_LCAP + 1, T - 1, T, T + 1):
        _check_cap(seq, k, FULL, want, cap)
    mh = so.max_hash_for_scaled(50)     # every workgroup's hashes fit its LDS list: all go through the flush
    want50 = want[want <= np.uint64(mh)]
    assert 0 < want50.size < SK_LCAP
    for cap in (want50.size // 2, want50.size):
        _check_cap(seq, k, mh, want50, cap)


@pytest.mark.gpu
def test_t6_cap_host(hip_lib):
    from yacht_amd import _lib, sketch

    k = 31
    seq = np.ascontiguousarray(random_bases(T6_N, T6_SEED))
    want = np.sort(base_hashes(T6_N, T6_SEED, k))
    T = want.size
    n_out = C.c_uint64(12345)
    small = np.full(T - 1 + CANARY, PREFILL, dtype=np.uint64)
    rc = hip_lib.yh_sketch_dna(C.c_void_p(seq.ctypes.data), seq.size, k, 42, FULL, 0, T - 1, C.c_void_p(small.ctypes.data), C.byref(n_out))
    assert rc == _lib.YH_ERR_CAPACITY and n_out.value == T
    assert bool(np.all(small[T - 1:] == np.uint64(PREFILL)))
    n_out = C.c_uint64(12345)
    rc = hip_lib.yh_sketch_dna(C.c_void_p(seq.ctypes.data), seq.size, k, 42, FULL, 0, 0, None, C.byref(n_out))
    assert rc == _lib.YH_OK and n_out.value == T
    exact = np.full(T + CANARY, PREFILL, dtype=np.uint64)
    rc = hip_lib.yh_sketch_dna(C.c_void_p(seq.ctypes.data), seq.size, k, 42, FULL, 0, T, C.c_void_p(exact.ctypes.data), C.byref(n_out))
    assert rc == _lib.YH_OK and n_out.value == T
    assert np.array_equal(np.sort(exact[:T]), want) and bool(np.all(exact[T:] == np.uint64(PREFILL)))
    # hash_kmers starts from a buffer that is too small at scaled = 1 and asks again
    assert np.array_equal(np.sort(sketch.hash_kmers([seq], k, 1)), want)


# ---- T7: threshold and seed --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_t7_max_hash_is_inclusive(hip_lib):
    k, n = 31, 5000
    seq = random_bases(n, 707)
    H = np.sort(base_hashes(n, 707, k))
    for shift in (0, 9):        # both kernels have their own comparison
        for v in (H[0], H[H.size // 2], H[-1]):
            v = int(v)
            assert v > 0
            check_against(H[H <= np.uint64(v)], seq, k, ("<=", v, shift), max_hash=v, shift=shift)
            check_against(H[H < np.uint64(v)], seq, k, ("<", v, shift), max_hash=v - 1, shift=shift)
        check_against(H[H == np.uint64(0)], seq, k, ("0", shift), max_hash=0, shift=shift)
    seq40 = random_bases(n, 707)
    H40 = np.sort(base_hashes(n, 707, 40))
    v = int(H40[H40.size // 2])
    check_against(H40[H40 <= np.uint64(v)], seq40, 40, ("<=", 40), max_hash=v)
    check_against(H40[H40 < np.uint64(v)], seq40, 40, ("<", 40), max_hash=v - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 40, 70])
def test_t7_seeds(hip_lib, k):
    seq = random_bases(5000, 707)
    seen = []
    for seed in (0, 1, 42, 2 ** 32 + 5, 2 ** 64 - 1):
        want = oracle_hashes(seq, k, seed)
        check_against(want, seq, k, (k, seed), seed=seed)
        if k <= 64:
            check_against(want, seq, k, (k, seed, "byte-wise"), seed=seed, shift=2)
        seen.append(want)
    assert all(not np.array_equal(seen[0], s) for s in seen[1:])


# ---- T8: seeded fuzz ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("part", range(4))
def test_t8_fuzz(hip_lib, part):
    cases = fuzz_cases()
    assert len(cases) == FUZZ_CASES
    for i in range(part, FUZZ_CASES, 4):
        c = cases[i]
        want = np.sort(fuzz_expected(c)[0])
        check_against(want, c["seq"], c["k"], (i, c["k"], c["n"], c["shift"], c["scaled"]), seed=c["seed"],
                      max_hash=so.max_hash_for_scaled(c["scaled"]), shift=c["shift"])


# ---- T9: the host path -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_t9_host_buffers_are_reused_across_calls(hip_lib):
    from yacht_amd import sketch

    for n, k, scaled in ((200_000, 31, 100), (1_000, 21, 1), (0, 31, 1), (300_000, 51, 10), (1_000, 70, 1)):
        seq = random_bases(n, 900 + k).copy()
        seq[n // 3:n // 3 + 2] = ord("N")
        want = oracle_hashes(seq, k, 42, so.max_hash_for_scaled(scaled))
        assert (want.size > 0) == (n > 0)
        assert np.array_equal(np.sort(sketch.hash_kmers([seq.tobytes()], k, scaled)), want), (n, k, scaled)


@pytest.mark.gpu
def test_t9_records(hip_lib):
    from yacht_amd import sketch

    k = 31
    rng = np.random.default_rng(909)
    genome = random_bases(3000, 910, True)
    lengths = rng.integers(30, 161, size=500)
    lengths[:3] = (30, 31, 32)
    starts = rng.integers(0, genome.size - 160, size=500)
    reads = [genome[s:s + l].tobytes() for s, l in zip(starts, lengths)]
    assert min(map(len, reads)) < k and k in set(map(len, reads)) and max(map(len, reads)) > k
    for scaled in (1, 5):
        want_m, want_a = so.sketch_records(reads, k, scaled)
        assert want_m.size > 0 and int(want_a.max()) > 1
        got_m, got_a = sketch.sketch_sequences(reads, k, scaled)
        assert np.array_equal(got_m, want_m) and np.array_equal(got_a, want_a)
        got_m, got_a = sketch.sketch_sequences([np.frombuffer(r, dtype=np.uint8) for r in reads], k, scaled)
        assert np.array_equal(got_m, want_m) and np.array_equal(got_a, want_a)
    one = np.frombuffer(reads[-1], dtype=np.uint8)
    assert np.array_equal(np.sort(sketch.hash_kmers([one], k, 1)), oracle_hashes(one, k))
    assert sketch.hash_kmers([], k, 1).size == 0
    got_m, got_a = sketch.sketch_sequences([], k, 1)
    assert got_m.size == 0 and got_a.size == 0
    assert got_m.dtype == np.uint64 and got_a.dtype == np.int64


# ---- T10: refusals that launch nothing ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_t10_refusals(hip_lib):
    import torch

    from yacht_amd import _lib

    seq = random_bases(1000, 1010)
    for k in (0, -1, 256):
        count, stored, canary = dev_sketch(seq, k, cap=16, expect_rc=_lib.YH_ERR_INVALID_ARG)
        assert count == -1      # d_count as the helper left it: not even zeroed
        assert bool(np.all(stored == np.uint64(PREFILL))) and bool(np.all(canary == np.uint64(PREFILL)))
    d_seq = torch.from_numpy(np.array(seq)).cuda()
    out = torch.full((16,), PREFILL - 2 ** 64, dtype=torch.int64, device="cuda")
    rc = hip_lib.yh_sketch_dna_device(C.c_void_p(d_seq.data_ptr()), seq.size, 31, 42, FULL, 16, C.c_void_p(out.data_ptr()), None,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.YH_ERR_INVALID_ARG
    assert bool(np.all(out.cpu().numpy().view(np.uint64) == np.uint64(PREFILL)))
