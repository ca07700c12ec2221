"""FracMinHash sketching of DNA on the HIP engine.

The reference's `yacht sketch ref|sample` are thin wrappers around the third-party
`sourmash sketch dna -p k=K,scaled=S,abund` (src/yacht/sketch_ref_genomes.py:24-61,
sketch_sample.py:31-49).  Here the k-mer hashing runs in libyacht_hip.so (yh_sketch_dna) and this
module does the file handling: FASTA/FASTQ (optionally gzip) in, sourmash-format signatures out
(yacht_amd.sigio), one signature per file (all records merged) like `sourmash sketch` without
`--singleton`.  `yacht sketch ref` sends many records or genome files through ONE device call
(yh_sketch_segments: one segment, one finished sketch each); `yacht sketch sample` streams its read files, chunk by
chunk, through ONE device accumulator (yh_sketch_acc) that keeps the distinct hashes and their counts in HBM.
"""
from __future__ import annotations

import ctypes as C
import gzip
import os
import queue
import threading
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, sigio

DEFAULT_SEED = 42


def max_hash_for_scaled(scaled: int) -> int:
    """sourmash: floor(float(2**64 - 1) / scaled); 18446744073709552 for scaled = 1000."""
    return int(float(2 ** 64 - 1) / float(scaled)) if scaled > 1 else 2 ** 64 - 1


def read_sequences(path: str) -> Iterator[Tuple[str, bytes]]:
    """(name, sequence) records of a FASTA or FASTQ file, gzip or plain."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        first = f.read(1)
        if not first:
            return
        rest = f.read()
    data = first + rest
    if first == b"@":  # FASTQ: 4-line records
        lines = data.split(b"\n")
        for i in range(0, len(lines) - 1, 4):
            if lines[i].startswith(b"@"):
                yield lines[i][1:].decode("utf-8", "replace"), lines[i + 1].strip()
        return
    name, parts = None, []
    for line in data.split(b"\n"):
        line = line.rstrip()
        if line.startswith(b">"):
            if name is not None:
                yield name, b"".join(parts)
            name, parts = line[1:].decode("utf-8", "replace"), []
        elif line:
            parts.append(line)
    if name is not None:
        yield name, b"".join(parts)


def hash_kmers(sequences: Iterable[bytes], ksize: int, scaled: int, seed: int = DEFAULT_SEED,
               device: int = 0) -> np.ndarray:
    """Kept hashes (unsorted, with duplicates) of all windows of all sequences: one device call on
    the sequences joined by a separator byte (a non-ACGT byte breaks every window that spans it)."""
    lib = _lib.load()
    seqs = list(sequences)
    if len(seqs) == 1:  # (no copy: a genome of one record, or a caller that joined the records itself)
        buf = seqs[0] if isinstance(seqs[0], np.ndarray) else np.frombuffer(seqs[0], dtype=np.uint8)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
    else:
        buf = np.frombuffer(b"\n".join(bytes(s) for s in seqs), dtype=np.uint8)
    if buf.size < ksize:
        return np.zeros(0, dtype=np.uint64)
    mh = max_hash_for_scaled(scaled)
    cap = max(int(buf.size / max(scaled, 1) * 1.5) + 4096, 4096)
    n = C.c_uint64(0)
    while True:
        out = np.empty(cap, dtype=np.uint64)
        rc = lib.yh_sketch_dna(C.c_void_p(buf.ctypes.data), buf.size, ksize, seed, mh, device, cap,
                               C.c_void_p(out.ctypes.data), C.byref(n))
        if rc == _lib.YH_ERR_CAPACITY:
            cap = int(n.value) + 16
            continue
        _lib.check(rc)
        return out[: int(n.value)]


def sketch_sequences(sequences: Iterable[bytes], ksize: int = 31, scaled: int = 1000, seed: int = DEFAULT_SEED,
                     device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(mins ascending, abundances) — what a sourmash signature stores."""
    kept = hash_kmers(sequences, ksize, scaled, seed, device)
    mins, counts = np.unique(kept, return_counts=True)
    return mins.astype(np.uint64), counts.astype(np.int64)


def sketch_file(path: str, ksize: int = 31, scaled: int = 1000, name: Optional[str] = None, seed: int = DEFAULT_SEED,
                device: int = 0) -> sigio.Signature:
    """One signature for the whole file; `name` defaults to the first record's header, as
    `sourmash sketch --name-from-first` does."""
    records = list(read_sequences(path))
    mins, ab = sketch_sequences((s for _n, s in records), ksize, scaled, seed, device)
    if name is None:
        name = records[0][0] if records else os.path.basename(path)
    mh = sigio.MinHash(mins, ksize, max_hash_for_scaled(scaled), ab, seed=seed)
    return sigio.Signature(mh, name=name, filename=path)


# ---- many records per device call (yh_sketch_segments) ----
SEGMENT_CALL_LIMIT = 2 ** 32          # bytes: a segmented call takes less than this
DEFAULT_BATCH_BYTES = 256 << 20       # of sequence per call (YACHT_SKETCH_BATCH_BYTES overrides it)
MAX_READERS = 16


def sketch_segments(buf, seg_off, ksize: int, scaled: int, seed: int = DEFAULT_SEED,
                    device: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One finished sketch per segment of `buf` in one device call: (mins uint64, abund uint32, off uint64[n_seg + 1]);
    segment s owns mins[off[s]:off[s + 1]], strictly ascending.  seg_off[n_seg + 1]: ascending byte offsets from 0 to
    len(buf).  A window counts for the segment its first byte lies in, and only when all its bytes lie inside it."""
    lib = _lib.load()
    if isinstance(buf, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(buf, dtype=np.uint8)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off_in = np.ascontiguousarray(seg_off, dtype=np.uint64)
    if off_in.ndim != 1 or off_in.size < 1:
        raise ValueError("seg_off needs n_seg + 1 entries")
    n_seg = off_in.size - 1
    mh = max_hash_for_scaled(scaled)
    cap = min(int(buf.size / max(scaled, 1) * 1.5) + 4096, max(int(buf.size), 1))
    off = np.empty(n_seg + 1, dtype=np.uint64)
    n = C.c_uint64(0)
    while True:
        mins = np.empty(cap, dtype=np.uint64)
        abund = np.empty(cap, dtype=np.uint32)
        rc = lib.yh_sketch_segments(C.c_void_p(buf.ctypes.data), buf.size, C.c_void_p(off_in.ctypes.data), n_seg, ksize, seed, mh,
                                    device, cap, C.c_void_p(mins.ctypes.data), C.c_void_p(abund.ctypes.data),
                                    C.c_void_p(off.ctypes.data), C.byref(n))
        if rc == _lib.YH_ERR_CAPACITY:
            cap = int(n.value)
            continue
        _lib.check(rc)
        return mins[: int(n.value)], abund[: int(n.value)], off


def batch_bytes() -> int:
    v = os.environ.get("YACHT_SKETCH_BATCH_BYTES")
    return max(int(v), 1) if v else DEFAULT_BATCH_BYTES


def use_loop_path() -> bool:
    """YACHT_SKETCH_REF=loop: one device call per record / per file, for A/B checks against the batched path."""
    return os.environ.get("YACHT_SKETCH_REF", "") == "loop"


def sketch_units(units: Iterable[bytes], ksize: int, scaled: int, seed: int = DEFAULT_SEED, device: int = 0,
                 budget: Optional[int] = None) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
    """(mins, abundances) of every unit (one segment each: a record, or a file's records joined by a newline), in order,
    what sketch_sequences([unit]) gives.  Units are gathered up to `budget` bytes per device call; one that is larger goes
    alone, and one too large for a segmented call takes the unsegmented path.  `units` is consumed lazily, a batch at a
    time, so a producer that reads ahead (read_units_ahead) works while the device does."""
    budget = batch_bytes() if budget is None else budget
    batch: List[bytes] = []
    held = 0

    def flush():
        nonlocal batch, held
        if not batch:
            return
        off = np.zeros(len(batch) + 1, dtype=np.uint64)
        np.cumsum([len(u) for u in batch], out=off[1:])
        buf = np.frombuffer(b"".join(batch), dtype=np.uint8) if len(batch) > 1 else np.frombuffer(batch[0], dtype=np.uint8)
        mins, abund, o = sketch_segments(buf, off, ksize, scaled, seed, device)
        o = o.astype(np.int64)
        batch, held = [], 0
        for s in range(o.size - 1):
            yield mins[o[s]:o[s + 1]].copy(), abund[o[s]:o[s + 1]].astype(np.int64)

    for u in units:
        u = bytes(u) if not isinstance(u, bytes) else u
        if len(u) >= SEGMENT_CALL_LIMIT:
            yield from flush()
            yield sketch_sequences([u], ksize, scaled, seed, device)
            continue
        if batch and held + len(u) > min(budget, SEGMENT_CALL_LIMIT - 1):
            yield from flush()
        batch.append(u)
        held += len(u)
    yield from flush()


def _read_unit(path: str) -> Tuple[Optional[str], bytes]:
    """(first record's name, the file's records joined by a newline): a genome file as ONE segment"""
    records = list(read_sequences(path))
    return (records[0][0] if records else None), b"\n".join(s for _n, s in records)


def read_units_ahead(paths: Sequence[str], budget: int) -> Iterator[Tuple[Optional[str], bytes]]:
    """_read_unit of every path, in order, read and decompressed by a small thread pool that runs ahead of the consumer by
    about two batches (judged by file size; a gzip file counts four times): the next batch is read while the device works
    on the current one (gzip and file reads release the GIL)."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor

    if not paths:
        return

    def estimate(p):
        try:
            size = os.path.getsize(p)
        except OSError:
            size = 0
        return size * (4 if p.endswith(".gz") else 1)

    with ThreadPoolExecutor(max_workers=min(MAX_READERS, len(paths))) as pool:
        ahead: deque = deque()
        in_flight = 0
        nxt = 0
        while nxt < len(paths) or ahead:
            while nxt < len(paths) and (not ahead or in_flight < 2 * budget):
                est = estimate(paths[nxt])
                ahead.append((pool.submit(_read_unit, paths[nxt]), est))
                in_flight += est
                nxt += 1
            fut, est = ahead.popleft()
            in_flight -= est
            yield fut.result()


def sketch_genome_files(named_paths: Sequence[Tuple[Optional[str], str]], ksize: int, scaled: int,
                        device: int = 0) -> List[sigio.Signature]:
    """One signature per (name, path), in order -- what sketch_file(path, name=name) gives for each (name None: the first
    record's header) -- with many files per device call."""
    if use_loop_path():
        return [sketch_file(p, ksize, scaled, name=n, device=device) for n, p in named_paths]
    budget = batch_bytes()
    first_names: List[Optional[str]] = []

    def units():
        for first, joined in read_units_ahead([p for _n, p in named_paths], budget):
            first_names.append(first)
            yield joined

    sigs = []
    for i, (mins, ab) in enumerate(sketch_units(units(), ksize, scaled, device=device, budget=budget)):
        name, path = named_paths[i]
        if name is None:
            name = first_names[i] if first_names[i] is not None else os.path.basename(path)
        sigs.append(sigio.Signature(sigio.MinHash(mins, ksize, max_hash_for_scaled(scaled), ab, seed=DEFAULT_SEED), name=name, filename=path))
    return sigs


def sketch_files(paths: Sequence[str], out_zip: str, ksize: int = 31, scaled: int = 1000, device: int = 0) -> List[sigio.Signature]:
    """`yacht sketch ref`-style: one signature per genome file, written as a sourmash .sig.zip."""
    sigs = sketch_genome_files([(None, p) for p in paths], ksize, scaled, device=device)
    sigio.write_sig_zip(sigs, out_zip)
    return sigs


# ---- `yacht sketch ref` / `yacht sketch sample` (reference sketch_ref_genomes.py, sketch_sample.py) ----
GENOME_SUFFIXES = (".fasta", ".fna", ".fas", ".fa", ".fasta.gz", ".fna.gz", ".fas.gz", ".fa.gz")


def add_ref_arguments(parser) -> None:
    parser.add_argument("--infile", help="Input file or folder path.", required=True)
    parser.add_argument("--kmer", type=int, help="K-mer size.", default=31)
    parser.add_argument("--scaled", type=int, help="Scaled factor.", default=1000)
    parser.add_argument("--outfile", help="Output file name.", required=True)


def main_ref(args) -> None:
    """A file: one signature per record (the reference passes --singleton).  A folder: one
    signature per genome file found under it, named by the file name without its suffix.  Either way many records or
    files go through one device call (sketch_units); YACHT_SKETCH_REF=loop keeps one call per record / per file."""
    if os.path.isfile(args.infile):
        records = list(read_sequences(args.infile))
        if use_loop_path():
            sketches = (sketch_sequences([seq], args.kmer, args.scaled) for _name, seq in records)
        else:
            sketches = sketch_units((seq for _name, seq in records), args.kmer, args.scaled)
        sigs = [sigio.Signature(sigio.MinHash(mins, args.kmer, max_hash_for_scaled(args.scaled), ab), name=name, filename=args.infile)
                for (name, _seq), (mins, ab) in zip(records, sketches)]
    elif os.path.isdir(args.infile):
        found = []
        for root, _dirs, files in os.walk(args.infile):
            for f in sorted(files):
                for suf in GENOME_SUFFIXES:
                    if f.endswith(suf):
                        found.append((f[: -len(suf)], os.path.join(root, f)))
                        break
        sigs = sketch_genome_files(sorted(found), args.kmer, args.scaled)
    else:
        raise FileNotFoundError(f"Input path {args.infile} does not exist.")
    sigio.write_sig_zip(sigs, args.outfile)


def add_sample_arguments(parser) -> None:
    parser.add_argument("--infile", nargs="+", required=True,
                        help="Input FASTA/Q file(s). For paired-end reads, provide two files.")
    parser.add_argument("--kmer", type=int, help="K-mer size.", default=31)
    parser.add_argument("--scaled", type=int, help="Scaled factor.", default=1000)
    parser.add_argument("--outfile", help="Output file name.", required=True)


# ---- one sketch out of many chunks (yh_sketch_acc): what `yacht sketch sample` streams its read files through ----
class SketchAccumulator:
    """The distinct kept hashes of everything added so far, with their counts, held on the device (yh_sketch_acc_*).
    A chunk is records joined by a byte that is not a base; the result depends only on the multiset of kept hashes, not
    on the chunking or on `cap_entries` (the log's first capacity; 0: the library's default)."""

    def __init__(self, ksize: int, scaled: int = 1000, seed: int = DEFAULT_SEED, device: int = 0, cap_entries: int = 0,
                 max_hash: Optional[int] = None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.max_hash = max_hash_for_scaled(scaled) if max_hash is None else int(max_hash)
        _lib.check(self._lib.yh_sketch_acc_create(device, ksize, seed, self.max_hash, cap_entries, C.byref(self._h)))

    def _handle(self) -> C.c_void_p:
        if not self._h:
            raise _lib.YachtHipError(_lib.YH_ERR_INVALID_ARG, "the sketch accumulator is closed")
        return self._h

    def add(self, chunk) -> None:
        buf = chunk if isinstance(chunk, np.ndarray) else np.frombuffer(chunk, dtype=np.uint8)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        _lib.check(self._lib.yh_sketch_acc_add(self._handle(), C.c_void_p(buf.ctypes.data) if buf.size else None, buf.size))

    def add_device(self, d_ptr: int, n_bytes: int) -> None:
        """a chunk that is already in device memory (complete when the call is made)"""
        _lib.check(self._lib.yh_sketch_acc_add_device(self._handle(), C.c_void_p(d_ptr), n_bytes))

    def add_hashes(self, hashes, counts=None) -> None:
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        c = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint64)
        if c is not None and c.shape != h.shape:
            raise ValueError("hashes and counts differ in length")
        _lib.check(self._lib.yh_sketch_acc_add_hashes(self._handle(), C.c_void_p(h.ctypes.data) if h.size else None,
                                                      C.c_void_p(c.ctypes.data) if c is not None and c.size else None, h.size))

    def info(self) -> dict:
        i = _lib.SketchAccInfo()
        _lib.check(self._lib.yh_sketch_acc_get_info(self._handle(), C.byref(i)))
        return {f: int(getattr(i, f)) for f, _t in _lib.SketchAccInfo._fields_}

    def finish(self) -> Tuple[np.ndarray, np.ndarray]:
        """(mins strictly ascending, their summed counts), both uint64; the accumulator goes on"""
        n = C.c_uint64(0)
        _lib.check(self._lib.yh_sketch_acc_finish(self._handle(), 0, None, None, C.byref(n)))
        mins = np.empty(int(n.value), dtype=np.uint64)
        counts = np.empty(int(n.value), dtype=np.uint64)
        if mins.size:
            _lib.check(self._lib.yh_sketch_acc_finish(self._handle(), mins.size, C.c_void_p(mins.ctypes.data),
                                                      C.c_void_p(counts.ctypes.data), C.byref(n)))
        return mins, counts

    def finish_device(self) -> Tuple[int, int, int]:
        """(device address of the mins, of the counts, their number): valid until the next call on the accumulator"""
        m, a, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        _lib.check(self._lib.yh_sketch_acc_finish_device(self._handle(), C.byref(m), C.byref(a), C.byref(n)))
        return int(m.value or 0), int(a.value or 0), int(n.value)

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, C.c_void_p()
            self._lib.yh_sketch_acc_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


READ_BLOCK_BYTES = 8 << 20    # of file (decompressed) per read of iter_sequence_chunks
READ_AHEAD_CHUNKS = 2         # chunks the reader thread may hold ready while the device works on one
_ChunkQueue = queue.Queue


def iter_sequence_chunks(path: str, budget: int, block_bytes: int = READ_BLOCK_BYTES) -> Iterator[bytes]:
    """The sequences of read_sequences(path), in order, as buffers of WHOLE records joined by a newline, each of at most
    `budget` bytes (a longer record goes alone) -- read in blocks, so that memory is bounded by the budget and the longest
    record, not by the file.  What is carried from block to block is the unfinished line and, for FASTA, the lines of the
    current record.  read_sequences' rules, which need the global line index: the first byte decides the format; FASTQ line
    4 i + 1 is a sequence when line 4 i starts with '@' (stripped; the last line counts without a newline); FASTA lines are
    right-stripped, blank ones skipped, and whatever precedes the first '>' is dropped."""
    budget = max(int(budget), 1)
    pieces: List[bytes] = []   # of the chunk being gathered: it is b"\n".join(pieces),
    held = 0                   # this long

    def take(records: List[bytes]) -> Iterator[bytes]:
        nonlocal pieces, held
        if not records:
            return
        joined = b"\n".join(records)
        if held + len(joined) + (1 if pieces else 0) <= budget:  # (all of a block's records at once: the usual case)
            held += len(joined) + (1 if pieces else 0)
            pieces.append(joined)
            return
        for r in records:
            if pieces and held + 1 + len(r) > budget:
                yield b"\n".join(pieces)
                pieces, held = [], 0
            held += len(r) + (1 if pieces else 0)
            pieces.append(r)

    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        block = f.read(block_bytes)
        if not block:
            return
        fastq = block[:1] == b"@"
        carry: List[bytes] = []    # the unfinished line, in the pieces it arrived in
        g = 0                      # global index of the next line
        head_ok = False            # FASTQ: the last first-of-four line seen starts with '@'
        named, parts = False, []   # FASTA: a header has been seen; the lines of the current record

        def lines_in(lines: List[bytes]) -> List[bytes]:
            """the records that these consecutive lines (the first has index g) complete"""
            nonlocal g, head_ok, named, parts
            recs: List[bytes] = []
            if fastq:
                h0, s0 = (-g) % 4, (1 - g) % 4
                oks = [h.startswith(b"@") for h in lines[h0::4]]
                seqs = lines[s0::4]
                flags = ([head_ok] + oks) if s0 < h0 else oks   # (s0 < h0: the first sequence line's header came earlier)
                if all(flags[:len(seqs)]):
                    recs = [s.strip() for s in seqs]
                else:
                    recs = [s.strip() for ok, s in zip(flags, seqs) if ok]
                if oks:
                    head_ok = oks[-1]
            else:
                for line in lines:
                    line = line.rstrip()
                    if line.startswith(b">"):
                        if named:
                            recs.append(b"".join(parts))
                        named, parts = True, []
                    elif line:
                        parts.append(line)
            g += len(lines)
            return recs

        while block:
            if b"\n" in block:
                lines = (b"".join(carry) + block if carry else block).split(b"\n")
                carry = [lines.pop()]
                yield from take(lines_in(lines))
            else:
                carry.append(block)
            block = f.read(block_bytes)
        yield from take(lines_in([b"".join(carry)]))   # (the last line, with or without text)
        if not fastq and named:
            yield from take([b"".join(parts)])
    if pieces:
        yield b"\n".join(pieces)


def read_chunks_ahead(paths: Sequence[str], budget: int) -> Iterator[bytes]:
    """iter_sequence_chunks of every path, in order, produced by a reader thread that stays at most READ_AHEAD_CHUNKS chunks
    ahead of the consumer (a bounded queue: file reads and gzip release the GIL, so the next chunks are read and
    decompressed while the device hashes the current one)."""
    q = _ChunkQueue(maxsize=READ_AHEAD_CHUNKS)
    stop = threading.Event()
    done = object()

    def put(item) -> bool:
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def produce():
        try:
            for p in paths:
                for chunk in iter_sequence_chunks(p, budget):
                    if not put(chunk):
                        return
            put(done)
        except BaseException as e:  # (handed to the consumer, which raises it)
            put(e)

    t = threading.Thread(target=produce, name="yacht-sketch-reader", daemon=True)
    t.start()
    try:
        while True:
            item = q.get()
            if item is done:
                return
            if isinstance(item, BaseException):
                raise item
            yield item
    finally:
        stop.set()
        t.join()


def use_whole_sample_path() -> bool:
    """YACHT_SKETCH_SAMPLE=whole: every file read whole, one device call, the kept hashes sorted on the host -- for A/B
    checks against the streamed path."""
    return os.environ.get("YACHT_SKETCH_SAMPLE", "") == "whole"


def sketch_sample_files(paths: Sequence[str], ksize: int = 31, scaled: int = 1000, seed: int = DEFAULT_SEED, device: int = 0,
                        budget: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(mins ascending, abundances) of all reads of all files merged -- what sketch_sequences gives for their sequences --
    with the files streamed in chunks of `budget` bytes (default: batch_bytes()) through ONE device accumulator: host
    memory is bounded by the budget, the sort and the counting happen on the device."""
    budget = batch_bytes() if budget is None else budget
    with SketchAccumulator(ksize, scaled, seed, device) as acc:
        for chunk in read_chunks_ahead(list(paths), budget):
            acc.add(chunk)
        mins, counts = acc.finish()
    return mins, counts.astype(np.int64)


def main_sample(args) -> None:
    """All reads of the one or two files merged into ONE signature with abundances.  The files are streamed through a device
    accumulator (sketch_sample_files); YACHT_SKETCH_SAMPLE=whole reads them whole and makes one device call instead."""
    if len(args.infile) not in (1, 2):
        raise ValueError("Please provide either one file for single-end reads or two files for paired-end reads.")
    if use_whole_sample_path():
        seqs: List[bytes] = []
        for path in args.infile:
            seqs += [s for _n, s in read_sequences(path)]
        mins, ab = sketch_sequences(seqs, args.kmer, args.scaled)
    else:
        mins, ab = sketch_sample_files(args.infile, args.kmer, args.scaled)
    sig = sigio.Signature(sigio.MinHash(mins, args.kmer, max_hash_for_scaled(args.scaled), ab),
                          name=os.path.basename(args.infile[0]), filename=args.infile[0])
    sigio.write_sig_zip([sig], args.outfile)
