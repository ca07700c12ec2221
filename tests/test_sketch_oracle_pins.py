"""oracle/sketch_oracle.py pinned from outside, and the case lists of tests/test_gpu_sketch_edges.py checked for what they
must cover.  No GPU: SMHasher's published verification value for MurmurHash3_x64_128, a scalar restatement
(tests/sketch_scalar.py) against the vectorised oracle, and sketch.read_sequences on hand-written files."""
import gzip

import numpy as np
import pytest

import sketch_scalar as sc
import test_gpu_sketch_edges as edges
from oracle import sketch_oracle as so

SMHASHER_MURMUR3_X64_128 = 0x6384BA69   # SMHasher main.cpp, the entry of MurmurHash3_x64_128


def _smhasher_verification(hash128):
    """SMHasher's VerificationTest: keys {0, 1, .., i-1} for i in 0..255 hashed with seed 256 - i, the 256 digests
    hashed with seed 0, the first four bytes of that digest read little-endian"""
    key = bytes(range(256))
    digests = b""
    for i in range(256):
        h1, h2 = hash128(key[:i], 256 - i)
        digests += h1.to_bytes(8, "little") + h2.to_bytes(8, "little")
    assert len(digests) == 4096
    return hash128(digests, 0)[0] & 0xFFFFFFFF


def _numpy_hash128(b, seed):
    h1, h2 = so.murmur3_x64_128(np.frombuffer(b, dtype=np.uint8).reshape(1, len(b)), seed)
    return int(h1[0]), int(h2[0])


def test_smhasher_verification_value():
    assert _smhasher_verification(sc.murmur3_x64_128) == SMHASHER_MURMUR3_X64_128
    assert _smhasher_verification(_numpy_hash128) == SMHASHER_MURMUR3_X64_128


def test_h1_is_the_first_word():
    b = np.arange(5 * 37, dtype=np.uint8).reshape(5, 37)
    assert np.array_equal(so.murmur3_x64_128_h1(b, 7), so.murmur3_x64_128(b, 7)[0])
    assert sc.murmur3_x64_128(b"ACG", 42)[0] == 1731421407650554201    # sourmash's published hash_murmur("ACG")


def _same(seq, k, seed=42):
    got = so.kmer_hashes(bytes(seq), k, seed)
    want = sc.kmer_hashes(bytes(seq), k, seed)
    assert got.dtype == np.uint64 and got.tolist() == want, (k, seed)
    return len(want)


@pytest.mark.parametrize("k", [2, 4, 30, 31, 32, 34, 62, 64, 66, 254])
def test_scalar_equals_oracle_low_complexity(k):
    # (period <= 4: k + 12 bytes hold every distinct window of the 8192 + k + 100 the GPU test runs, several times over)
    for name, seq in edges.low_complexity(k, extra=12).items():
        assert edges.low_complexity(k)[name].startswith(seq)
        assert _same(seq, k) == 13


@pytest.mark.parametrize("k", [32, 64, 66])
def test_scalar_equals_oracle_palindromes(k):
    assert _same(edges.palindrome_family(k), k) == 3 * k + 1


def test_scalar_equals_oracle_small_fuzz_cases():
    small = [c for c in edges.fuzz_cases() if c["n"] <= 600]
    assert len(small) >= 30
    windows = 0
    for c in small:
        windows += _same(c["seq"].tobytes(), c["k"], c["seed"])
        assert np.array_equal(edges.valid_windows(c["seq"], c["k"]),
                              np.array([all(b in b"ACGTacgt" for b in c["seq"][i:i + c["k"]].tobytes())
                                        for i in range(max(c["n"] - c["k"] + 1, 0))], dtype=bool))
    assert windows > 100    # (the comparison is not vacuous)


def test_fuzz_case_list_covers_what_it_must():
    cases = edges.fuzz_cases()
    assert len(cases) == 300
    assert {c["k"] for c in cases} == set(edges.FUZZ_KS) and {c["scaled"] for c in cases} == {1, 3, 50}
    assert {c["shift"] for c in cases} == set(range(16))
    assert all(c["seq"].size == c["n"] and 0 <= c["n"] < 3 * 8192 for c in cases)
    on = {"64": 0, "128": 0, "bytes": 0}
    short = no_window = overflow = 0
    for c in cases:
        kernel = edges.kernel_of(c["k"], c["shift"])
        on[kernel] += 1
        kept, win = edges.fuzz_expected(c)
        if c["n"] < c["k"]:
            short += 1
        elif not edges.valid_windows(c["seq"], c["k"]).any():
            no_window += 1
        # the LDS list overflows only in the 2-bit kernels: a workgroup of the byte-wise one has 2048 windows in all
        if kernel != "bytes" and win.size and int(np.bincount(win // edges.RL_WIN).max()) > edges.SK_LCAP:
            overflow += 1
    assert min(on.values()) >= 40, on
    assert short >= 10 and no_window >= 10 and overflow >= 20, (short, no_window, overflow)


# ---- sketch.read_sequences ---------------------------------------------------------------------------------------------------
FASTA = (b">one first record\r\nACGT\r\nacgtn\r\n\r\n>empty\r\n>three\r\n\r\nGG\r\nTT",
         [("one first record", b"ACGTacgtn"), ("empty", b""), ("three", b"GGTT")])
FASTA_LF = (b">a\nAC\nGT\n\n>b\n>c d\nNNAC\n",
            [("a", b"ACGT"), ("b", b""), ("c d", b"NNAC")])
FASTQ = (b"@r1 x\nACGT\n+\n@III\n@r2\nGGNA\n+r2\n>@@I\n@r3\nTT\n+\nII\n",
         [("r1 x", b"ACGT"), ("r2", b"GGNA"), ("r3", b"TT")])
FASTQ_NO_NEWLINE = (b"@r1\nACGT\n+\n@>II\n@r2\nacg\n+\n>II",
                    [("r1", b"ACGT"), ("r2", b"acg")])


@pytest.mark.parametrize("name,content,want", [("a.fa", *FASTA), ("b.fna", *FASTA_LF), ("c.fq", *FASTQ),
                                               ("d.fastq", *FASTQ_NO_NEWLINE), ("e.fa", b"", [])])
def test_read_sequences(tmp_path, name, content, want):
    from yacht_amd import sketch

    plain = tmp_path / name
    plain.write_bytes(content)
    assert list(sketch.read_sequences(str(plain))) == want
    zipped = tmp_path / (name + ".gz")
    with gzip.open(zipped, "wb") as f:
        f.write(content)
    assert list(sketch.read_sequences(str(zipped))) == want
    if name.endswith((".fa", ".fna")):     # the oracle's own FASTA reader agrees
        assert list(so.read_fasta(str(plain))) == want
