"""Scalar restatement of the DNA FracMinHash hash, for the sketch tests.  Deliberately naive: Python ints and bytes, no
numpy, nothing shared with oracle/sketch_oracle.py.  MurmurHash3_x64_128 is written from the published algorithm
(Austin Appleby, public domain, MurmurHash3.cpp); the canonical k-mer is min(kmer, revcomp(kmer)) on Python bytes."""

M64 = (1 << 64) - 1
C1 = 0x87C37B91114253D5
C2 = 0x4CF5AD432745937F


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def murmur3_x64_128(key, seed):
    """(h1, h2) of MurmurHash3_x64_128 of the bytes `key`."""
    key = bytes(key)
    length = len(key)
    h1 = h2 = seed & M64
    nblocks = length // 16
    for i in range(nblocks):
        k1 = int.from_bytes(key[16 * i:16 * i + 8], "little")
        k2 = int.from_bytes(key[16 * i + 8:16 * i + 16], "little")
        k1 = (k1 * C1) & M64
        k1 = _rotl(k1, 31)
        k1 = (k1 * C2) & M64
        h1 ^= k1
        h1 = _rotl(h1, 27)
        h1 = (h1 + h2) & M64
        h1 = (h1 * 5 + 0x52DCE729) & M64
        k2 = (k2 * C2) & M64
        k2 = _rotl(k2, 33)
        k2 = (k2 * C1) & M64
        h2 ^= k2
        h2 = _rotl(h2, 31)
        h2 = (h2 + h1) & M64
        h2 = (h2 * 5 + 0x38495AB5) & M64
    tail = key[16 * nblocks:]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        k2 = (k2 * C2) & M64
        k2 = _rotl(k2, 33)
        k2 = (k2 * C1) & M64
        h2 ^= k2
    if len(tail) > 0:
        k1 = int.from_bytes(tail[:8], "little")
        k1 = (k1 * C1) & M64
        k1 = _rotl(k1, 31)
        k1 = (k1 * C2) & M64
        h1 ^= k1
    h1 ^= length
    h2 ^= length
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1 = _fmix(h1)
    h2 = _fmix(h2)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return h1, h2


_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
_BASES = frozenset(b"ACGTacgt")


def revcomp(kmer):
    return kmer.translate(_COMPLEMENT)[::-1]


def kmer_hashes(seq, ksize, seed=42):
    """list of the hashes of every valid window of `seq`, in window order."""
    seq = bytes(seq)
    out = []
    for i in range(len(seq) - ksize + 1):
        w = seq[i:i + ksize]
        if all(c in _BASES for c in w):
            w = w.upper()
            out.append(murmur3_x64_128(min(w, revcomp(w)), seed)[0])
    return out
