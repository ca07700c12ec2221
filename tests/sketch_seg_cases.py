"""Case builders for the segmented sketch (yh_sketch_segments*): buffers, segment tables and what the oracle says about
them.  No GPU is needed here; tests/test_sketch_seg_cases_cpu.py checks the expectations a second way and
tests/test_gpu_sketch_segments.py runs the cases on the device.

A case is a dict: name, buf (read-only uint8), seg_off (uint64[n_seg + 1]), k, scaled, shift (bytes the device pointer is
moved off its 16-byte alignment: anything but 0 reaches the byte-wise kernel) and small (cheap enough for the scalar
restatement)."""
import functools
import os

import numpy as np

import test_gpu_sketch_edges as edges
from oracle import sketch_oracle as so

# the geometry of yh_sketch.hip, by its names there
UNIT = 16              # bases per staged unit
RL_RUN = 32            # windows per lane of the 2-bit kernels
RL_WIN = 8192          # windows per workgroup of the 2-bit kernels
SK_WIN = 2048          # windows per workgroup of the byte-wise kernel
SK_LCAP = 2048         # kept hashes a workgroup parks in LDS before they overflow to global memory

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixtures")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _case(name, buf, seg_off, k, scaled, shift=0, small=False):
    buf = np.frombuffer(bytes(buf), dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.array(buf, dtype=np.uint8)
    buf.setflags(write=False)
    seg_off = np.asarray(seg_off, dtype=np.uint64)
    assert seg_off[0] == 0 and int(seg_off[-1]) == buf.size and bool(np.all(seg_off[1:] >= seg_off[:-1])), name
    seg_off.setflags(write=False)
    return dict(name=name, buf=buf, seg_off=seg_off, k=k, scaled=scaled, shift=shift, small=small)


def kernel_of(case):
    return edges.kernel_of(case["k"], case["shift"])


# ---- 1: boundaries against the kernel's grid -------------------------------------------------------------------------------
def _boundary_case(name, k, grid, shift, d):
    """touching segments whose boundaries sit d (-1, 0, +1) off a unit edge, a lane edge, and the first and second
    workgroup edge of a kernel with `grid` windows per workgroup; scaled 1: every window is emitted"""
    n = 2 * grid + 77
    lane_edge = 5 * RL_RUN if grid == SK_WIN else 100 * RL_RUN
    cuts = sorted({7 * UNIT + d, lane_edge + d, grid + d, grid + lane_edge + UNIT + d, 2 * grid + d})
    assert (7 * UNIT) % RL_RUN != 0 and lane_edge % RL_RUN == 0 and cuts[-1] < n
    seq = edges.random_bases(n, 1100 + k)
    return _case(name, seq, [0] + cuts + [n], k, 1, shift=shift)


def boundary_cases():
    out = []
    for k in (21, 32, 33, 51, 64):
        for d in (-1, 0, 1):
            out.append(_boundary_case(f"edge-k{k}-d{d:+d}", k, RL_WIN, 0, d))
    for k, shift in ((70, 0), (31, 1)):
        for d in (-1, 0, 1):
            out.append(_boundary_case(f"edge-bytes-k{k}-d{d:+d}", k, SK_WIN, shift, d))
    return out


# ---- 2: many tiny segments inside one workgroup's span ---------------------------------------------------------------------
def tiny_cases():
    out = []
    for k in (21, 33):
        lengths = [0] * 5 + [i % (k + 4) for i in range(3000)] + [0] * 5
        assert max(lengths) == k + 3 and sum(1 for x in lengths if x < k) > len(lengths) // 2
        off = np.concatenate(([0], np.cumsum(lengths)))
        seq = edges.random_bases(int(off[-1]), 1200 + k)
        out.append(_case(f"tiny-k{k}", seq, off, k, 1))
    return out


# ---- 3: duplicates and strands ---------------------------------------------------------------------------------------------
def strand_cases():
    k = 31
    x = edges.random_bases(3001, 1300).tobytes()
    rc = x.translate(_COMP)[::-1]
    assert rc != x
    first = x + b"N" + rc + b"N" + x
    dup = _case("strands-k31", first + x, [0, len(first), len(first) + len(x)], k, 1)
    fam = edges.palindrome_family(32)
    cut = len(fam) // 2
    pal = _case("palindromes-k32", fam, [0, cut, len(fam)], 32, 1, small=True)
    return [dup, pal]


# ---- 4: partial overflow of the LDS list -----------------------------------------------------------------------------------
def overflow_cases():
    n = 3 * RL_WIN
    seq = edges.random_bases(n, 1400).copy()
    seq[RL_WIN + 5000:RL_WIN + 5800] = ord("N")   # the second workgroup keeps a tenth fewer: below the list's size at scaled 4
    off = [0, 1000, RL_WIN - 3, RL_WIN + 4000, 2 * RL_WIN + 9, n]
    return [_case(f"overflow-s{scaled}", seq, off, 31, scaled) for scaled in (2, 4)]


def low_complexity_case():
    """a repeat whose few k-mers ALL hash under the threshold of scaled 2: twice the kept hashes a random sequence gives
    (the host form sizes its pair buffer for 1.25 x the random expectation and must notice)"""
    k, n = 31, 20_000
    mh = np.uint64(so.max_hash_for_scaled(2))
    for unit in (b"A", b"C", b"AC", b"AG", b"AT", b"CG", b"AAC", b"AAG", b"AAT", b"ACC", b"ACG", b"ACT", b"AGC", b"AGG", b"ATC"):
        seq = (unit * (n // len(unit) + 1))[:n]
        if bool(np.all(so.kmer_hashes(seq[:k + 8], k) <= mh)):
            return _case("lowcomplex-s2", seq, [0, 7000, n], k, 2)
    raise AssertionError("no repeat unit found")


# ---- 5: real data ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real_records():
    """the first records of two fixture genomes, about 100 kb of each (the last one cut)"""
    recs = []
    for f in ("GCF_018918045.1_genomic.fna.gz", "GCF_018918095.1_genomic.fna.gz"):
        room = 100_000
        for _name, s in so.read_fasta(os.path.join(FX, f)):
            recs.append(s[:room])
            room -= len(recs[-1])
            if room <= 0:
                break
    return tuple(recs)


def real_cases():
    recs = _real_records()
    off = np.concatenate(([0], np.cumsum([len(r) for r in recs])))
    return [_case(f"real-s{scaled}", b"".join(recs), off, 31, scaled) for scaled in (100, 1000)]


# ---- small ones for the scalar restatement ---------------------------------------------------------------------------------
def small_cases():
    out = []
    for k in (5, 21):
        lengths = [0, 0, k - 1, k, k + 1, 0, 3 * k, 1, 2 * k + 3, 0]
        off = np.concatenate(([0], np.cumsum(lengths)))
        seq = edges.random_bases(int(off[-1]), 1500 + k, True).copy()
        seq[int(off[6]) + k + 1] = ord("N")
        out.append(_case(f"small-k{k}", seq, off, k, 1, small=True))
        out.append(_case(f"small-k{k}-s3", seq, off, k, 3, small=True))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = boundary_cases() + tiny_cases() + strand_cases() + overflow_cases() + [low_complexity_case()] + real_cases() + small_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return tuple(cases)


def case_named(name):
    return next(c for c in all_cases() if c["name"] == name)


def segments(case):
    o = case["seg_off"].astype(np.int64)
    b = case["buf"].tobytes()
    return [b[o[s]:o[s + 1]] for s in range(o.size - 1)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(mins uint64, abund uint32, off uint64[n_seg + 1]) of a case by the oracle: kmer_hashes of every segment on its own,
    thresholded, np.unique with counts.  Read-only, computed once."""
    case = case_named(name)
    mh = np.uint64(so.max_hash_for_scaled(case["scaled"]))
    mins, abund, off = [], [], [0]
    for seg in segments(case):
        h = so.kmer_hashes(seg, case["k"])
        m, c = np.unique(h[h <= mh], return_counts=True)
        mins.append(m.astype(np.uint64))
        abund.append(c.astype(np.uint32))
        off.append(off[-1] + m.size)
    out = (np.concatenate(mins) if mins else np.zeros(0, np.uint64), np.concatenate(abund) if abund else np.zeros(0, np.uint32),
           np.array(off, dtype=np.uint64))
    for a in out:
        a.setflags(write=False)
    return out


def kept_total(name):
    """number of kept hashes (with duplicates) of a case = the sum of its abundances"""
    return int(expected(name)[1].sum())
