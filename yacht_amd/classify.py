"""`yacht classify`: a taxon for every contig, bin or read, against the database `yacht train` built.

`yacht run --lineages` gives the lowest common ancestor (LCA) of every SAMPLE hash and sums them per taxon.  This command asks
the same question per RECORD of a FASTA / FASTQ file: every record is sketched, its hashes are looked up in the resident
database, and the LCA of the hits that say something (those that resolve below the root) is the record's taxon -- what
`sourmash lca classify` does per signature.  (No reference counterpart; nearest elsewhere: `sourmash lca classify`.)

The device does all of it per chunk of records in one call (RefDB.classify_segments / yh_classify_segments): the records are
sketched as segments of one buffer, their sketches stay in HBM, and one row of four numbers per record comes back.
YACHT_CLASSIFY=loop is the A/B route: the existing segmented sketch, the existing RefDB.lca per non-empty record, the fold on
the host.  Both routes write the same files byte for byte.

Out of scope: Kraken's root-to-leaf path score, per-lineage thresholds, writing the classified sequences out, hash-range
shards, cohorts.
"""
from __future__ import annotations

import gzip
import json
import os
import queue
import threading
from pathlib import Path
from typing import Iterator, List, Sequence, Tuple

import numpy as np

from . import _lib, phases, sketch, taxonomy
from .utils import logger

RECORDS_NAME = "classify_records.tsv"
SUMMARY_NAME = "classify_summary.tsv"
RECORD_COLUMNS = ["file", "record", "length", "n_hashes", "n_hashes_in_database", "n_hashes_at_root", "status", "rank", "lineage"]
SUMMARY_COLUMNS = ["rank", "lineage", "n_records_direct", "n_records_clade", "bases_direct", "bases_clade", "f_records_clade",
                   "f_bases_clade"]
STATUS_COLUMNS = ["status", "n_records", "bases"]
NO_HASHES, NOT_IN_DATABASE, UNINFORMATIVE, BELOW_MIN_HITS, CONFLICT, CLASSIFIED = (
    "no_hashes", "not_in_database", "uninformative", "below_min_hits", "conflict", "classified")
STATUSES = (NO_HASHES, NOT_IN_DATABASE, UNINFORMATIVE, BELOW_MIN_HITS, CONFLICT, CLASSIFIED)
ROUTE_ENV = "YACHT_CLASSIFY"
RECORD_LIMIT = 2 ** 32 - 1  # bytes: a record of a segmented call is shorter than this

MSG_NO_CONFIG = "Config file {0} does not exist. Please run `yacht train` first."
MSG_NO_MANIFEST = "The manifest file {0} does not exist. Please check if you are using the correct json file as input."
MSG_NO_LINEAGES = "--lineages file {0} does not exist."
MSG_MIN_HITS = "--min_hits must be at least 1, not {0}."
MSG_NO_INFILE = "yacht classify needs at least one --infile."
MSG_NO_INPUT_FILE = "--infile {0} does not exist."
MSG_SAME_STEM = "--infile {0} and {1} have the same stem {2}: the `file` column could not tell their records apart."
MSG_BAD_ROUTE = "YACHT_CLASSIFY={0} is not a route: unset it, or set it to `loop`."
MSG_RECORD_TOO_LONG = "Record {0} of {1} holds {2} bases: a record must be shorter than 2**32 - 1 bytes."


def add_arguments(parser) -> None:
    parser.add_argument("--json", type=str, required=True, help="Config json written by `yacht train`.")
    parser.add_argument("--lineages", type=str, required=True,
                        help="A lineage table of the reference organisms (ident,superkingdom,...,species[,strain]), as for `yacht run --lineages`.")
    parser.add_argument("--infile", nargs="+", default=None, help="FASTA / FASTQ file(s), plain or gzip: every record is classified.")
    parser.add_argument("--outdir", type=str, default=os.getcwd(), help="Where the 'results' folder is created.")
    parser.add_argument("--min_hits", type=int, default=2,
                        help="A record is classified only when at least this many of its hashes resolve below the root.")
    parser.add_argument("--num_threads", type=int, default=16, help="Host threads for file handling.")


def file_stem(path: str) -> str:
    """The `file` column: the basename without .gz and without its last suffix."""
    name = os.path.basename(path)
    if name.endswith(".gz"):
        name = name[:-3]
    return os.path.splitext(name)[0]


def use_loop_route() -> bool:
    """YACHT_CLASSIFY=loop: sketch, one RefDB.lca per record, fold on the host.  ValueError for any other word."""
    word = os.environ.get(ROUTE_ENV, "")
    if word not in ("", "loop"):
        raise ValueError(MSG_BAD_ROUTE.format(word))
    return word == "loop"


# ---- the reader: records, not merged sequence ------------------------------------------------------------------------------------
def iter_records(path: str) -> Iterator[Tuple[str, bytes]]:
    """The (name, sequence) records of sketch.read_sequences(path), in its order and by its rules, read line by line: memory
    is bounded by the longest record, not by the file.  The first byte decides the format.  FASTQ: line 4 i is a header when
    it starts with '@' and a newline ends it, line 4 i + 1 (stripped) its sequence.  FASTA: lines are right-stripped, blank
    ones skipped, and whatever precedes the first '>' is dropped."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        first = f.readline()
        if not first:
            return
        if first[:1] == b"@":
            g, pending = 0, None
            line = first
            while line:
                if g % 4 == 0:
                    if pending is not None:  # (never: a header's sequence line follows it at once)
                        yield pending, b""
                    pending = line[1:-1].decode("utf-8", "replace") if line.startswith(b"@") and line.endswith(b"\n") else None
                elif g % 4 == 1 and pending is not None:
                    yield pending, (line[:-1] if line.endswith(b"\n") else line).strip()
                    pending = None
                g += 1
                line = f.readline()
            if pending is not None:  # (the file ends behind a header's newline: an empty sequence)
                yield pending, b""
            return
        name, parts = None, []
        line = first
        while line:
            line = line.rstrip()
            if line.startswith(b">"):
                if name is not None:
                    yield name, b"".join(parts)
                name, parts = line[1:].decode("utf-8", "replace"), []
            elif line:
                parts.append(line)
            line = f.readline()
        if name is not None:
            yield name, b"".join(parts)


def iter_record_chunks(path: str, budget: int):
    """(names, lengths int64 [n], buf uint8 -- the sequences one behind the other, no separator --, seg_off uint64 [n + 1]) per
    chunk of WHOLE records of at most `budget` bytes (a longer record goes alone).  ValueError for a record too long for a
    segmented call."""
    budget = max(int(budget), 1)
    names: List[str] = []
    seqs: List[bytes] = []
    held = 0

    def flush():
        nonlocal names, seqs, held
        lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lengths, out=off[1:])
        out = (names, lengths, np.frombuffer(b"".join(seqs), dtype=np.uint8), off)
        names, seqs, held = [], [], 0
        return out

    for name, seq in iter_records(path):
        if len(seq) >= RECORD_LIMIT:
            raise ValueError(MSG_RECORD_TOO_LONG.format(name.split()[0] if name.split() else "", path, len(seq)))
        if seqs and held + len(seq) > min(budget, RECORD_LIMIT - 1):
            yield flush()
        names.append(name)
        seqs.append(seq)
        held += len(seq)
    if seqs:
        yield flush()


def read_record_chunks_ahead(paths: Sequence[str], budget: int):
    """(index of the path, *chunk) for iter_record_chunks of every path, in order, from a reader thread that stays at most
    sketch.READ_AHEAD_CHUNKS chunks ahead of the consumer (as sketch.read_chunks_ahead)."""
    q: queue.Queue = queue.Queue(maxsize=sketch.READ_AHEAD_CHUNKS)
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
            for i, p in enumerate(paths):
                for chunk in iter_record_chunks(p, budget):
                    if not put((i,) + chunk):
                        return
            put(done)
        except BaseException as e:  # (handed to the consumer, which raises it)
            put(e)

    t = threading.Thread(target=produce, name="yacht-classify-reader", daemon=True)
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


# ---- rows -> status, tables ------------------------------------------------------------------------------------------------------
def status_of(rows, min_hits: int) -> np.ndarray:
    """The status of every row of engine.CLASSIFY_ROW_DTYPE (an object array of the STATUSES).  With i = n_hit - n_root:
    no_hashes (n_kept == 0), not_in_database (n_hit == 0), uninformative (i == 0), below_min_hits (0 < i < min_hits), conflict
    (i >= min_hits and the fold is the root), classified (i >= min_hits and the fold is below the root)."""
    n_kept = rows["n_kept"].astype(np.int64)
    n_hit = rows["n_hit"].astype(np.int64)
    inf = n_hit - rows["n_root"].astype(np.int64)
    out = np.full(rows.size, CLASSIFIED, dtype=object)
    out[rows["node"] == 0] = CONFLICT
    out[inf < int(min_hits)] = BELOW_MIN_HITS
    out[inf == 0] = UNINFORMATIVE
    out[n_hit == 0] = NOT_IN_DATABASE
    out[n_kept == 0] = NO_HASHES
    return out


def records_frame(files, names, lengths, rows, status, node_lineages):
    import pandas as pd

    classified = status == CLASSIFIED
    lin = [node_lineages[int(v)] if c else () for v, c in zip(rows["node"], classified)]
    return pd.DataFrame({
        "file": np.asarray(files, dtype=object),
        "record": np.asarray([n.split()[0] if n.split() else "" for n in names], dtype=object),
        "length": np.asarray(lengths, dtype=np.int64),
        "n_hashes": rows["n_kept"].astype(np.int64),
        "n_hashes_in_database": rows["n_hit"].astype(np.int64),
        "n_hashes_at_root": rows["n_root"].astype(np.int64),
        "status": status,
        "rank": np.asarray([taxonomy.RANKS[len(p) - 1] if p else "" for p in lin], dtype=object),
        "lineage": np.asarray([";".join(p) for p in lin], dtype=object),
    }, columns=RECORD_COLUMNS)


def summary_tables(parent, node_lineages, lengths, rows, status):
    """(status frame, taxon frame) of classify_summary.tsv: one row per status other than `classified` with its records and
    bases; then the root and every taxon with a non-zero clade, ordered by lineage as lca_summary.tsv orders them.  The
    fractions are over all records and all bases; the status rows plus the root's clade add up to the input."""
    import pandas as pd

    lengths = np.asarray(lengths, dtype=np.int64)
    n_nodes = len(node_lineages)
    n_all, b_all = int(lengths.size), int(lengths.sum())
    stat_rows = [[s, int((status == s).sum()), int(lengths[status == s].sum())] for s in STATUSES if s != CLASSIFIED]
    cl = status == CLASSIFIED
    direct = np.zeros((n_nodes, 2), dtype=np.uint64)
    if cl.any():
        nodes = rows["node"][cl].astype(np.int64)
        direct[:, 0] = np.bincount(nodes, minlength=n_nodes).astype(np.uint64)
        direct[:, 1] = np.bincount(nodes, weights=lengths[cl].astype(np.float64), minlength=n_nodes).astype(np.uint64)
    clade = taxonomy.clade_sums(parent, direct)
    tax_rows = []
    for v in sorted(range(n_nodes), key=lambda v: tuple(node_lineages[v])):
        if v != 0 and clade[v, 0] == 0:
            continue
        lin = node_lineages[v]
        tax_rows.append([taxonomy.RANKS[len(lin) - 1] if lin else taxonomy.ROOT, ";".join(lin), int(direct[v, 0]), int(clade[v, 0]),
                         int(direct[v, 1]), int(clade[v, 1]), int(clade[v, 0]) / n_all if n_all else 0.0,
                         int(clade[v, 1]) / b_all if b_all else 0.0])
    return pd.DataFrame(stat_rows, columns=STATUS_COLUMNS), pd.DataFrame(tax_rows, columns=SUMMARY_COLUMNS)


def write_outputs(results_folder: str, records, status_frame, taxon_frame) -> None:
    records.to_csv(os.path.join(results_folder, RECORDS_NAME), sep="\t", index=False)
    with open(os.path.join(results_folder, SUMMARY_NAME), "w", newline="") as f:
        status_frame.to_csv(f, sep="\t", index=False, lineterminator="\n")
        taxon_frame.to_csv(f, sep="\t", index=False, lineterminator="\n")


# ---- the two routes --------------------------------------------------------------------------------------------------------------
def _host_lca(parent, depth, a: int, b: int) -> int:
    while a != b:
        if depth[a] >= depth[b]:
            a = int(parent[a])
        else:
            b = int(parent[b])
    return a


def classify_chunk_loop(db, parent, depth, buf, seg_off, ksize: int, scaled: int) -> np.ndarray:
    """The rows of RefDB.classify_segments by the existing calls: sketch.sketch_segments, RefDB.lca per non-empty record, the
    fold on the host."""
    from .engine import CLASSIFY_ROW_DTYPE

    mins, _abund, off = sketch.sketch_segments(buf, seg_off, ksize, scaled)
    off = off.astype(np.int64)
    rows = np.zeros(off.size - 1, dtype=CLASSIFY_ROW_DTYPE)
    rows["node"] = _lib.YH_LCA_NONE
    for s in range(off.size - 1):
        n = int(off[s + 1] - off[s])
        rows["n_kept"][s] = n
        if n == 0:
            continue
        nodes, _counts = db.lca(mins[off[s]:off[s + 1]])
        hit = nodes[nodes != _lib.YH_LCA_NONE]
        rows["n_hit"][s] = hit.size
        rows["n_root"][s] = int((hit == 0).sum())
        inf = np.unique(hit[hit != 0])
        if inf.size:
            acc = int(inf[0])
            for v in inf[1:]:
                acc = _host_lca(parent, depth, acc, int(v))
            rows["node"][s] = acc
        elif hit.size:
            rows["node"][s] = 0
    return rows


def check_options(args) -> Tuple[List[str], bool]:
    """(input files, loop route), or ValueError / FileNotFoundError with a MSG_* text: before any device work or file."""
    files = getattr(args, "infile", None)
    files = [files] if isinstance(files, str) else list(files or [])
    if not files:
        raise ValueError(MSG_NO_INFILE)
    if int(args.min_hits) < 1:
        raise ValueError(MSG_MIN_HITS.format(args.min_hits))
    loop = use_loop_route()
    stems = {}
    for p in files:
        stem = file_stem(p)
        if stem in stems:
            raise ValueError(MSG_SAME_STEM.format(stems[stem], p, stem))
        stems[stem] = p
    if not os.path.isfile(str(args.json)):
        raise FileNotFoundError(MSG_NO_CONFIG.format(args.json))
    if not os.path.isfile(str(args.lineages)):
        raise FileNotFoundError(MSG_NO_LINEAGES.format(args.lineages))
    with open(str(args.json)) as f:
        manifest_path = json.load(f)["manifest_file_path"]
    if not os.path.isfile(manifest_path):
        raise FileNotFoundError(MSG_NO_MANIFEST.format(manifest_path))
    for p in files:
        if not os.path.isfile(p):
            raise FileNotFoundError(MSG_NO_INPUT_FILE.format(p))
    return files, loop


def main(args) -> None:
    import pandas as pd

    from . import hypothesis_recovery_src as hr

    files, loop = check_options(args)
    with open(str(Path(args.json).absolute())) as f:
        config = json.load(f)
    manifest_path, genome_dir = config["manifest_file_path"], config["intermediate_files_dir"]
    scale, ksize = int(config["scale"]), int(config["ksize"])
    lineages = taxonomy.read_lineages(str(args.lineages))
    results_folder = os.path.join(str(Path(args.outdir).absolute()), "results")
    os.makedirs(results_folder, exist_ok=True)
    with phases.phase("load_manifest"):
        manifest = pd.read_csv(manifest_path, sep="\t", header=0)
    parent, depth, leaf, node_lineages, _n_unmatched = taxonomy.build_tree(manifest["organism_name"], lineages)
    try:
        db = hr.get_reference_db(manifest, genome_dir, ksize, args.num_threads)
        with phases.phase("set_taxonomy"):
            db.set_taxonomy(parent, depth, leaf)
        stems = [file_stem(p) for p in files]
        col_file: List[str] = []
        col_name: List[str] = []
        col_len: List[np.ndarray] = []
        col_rows: List[np.ndarray] = []
        n_chunks = n_kept = 0
        with phases.phase("classify"):
            for i, names, lengths, buf, seg_off in read_record_chunks_ahead(files, sketch.batch_bytes()):
                if loop:
                    rows = classify_chunk_loop(db, parent, depth, buf, seg_off, ksize, scale)
                else:
                    rows = db.classify_segments(buf, seg_off, ksize, scale)
                n_chunks += 1
                n_kept += int(rows["n_kept"].sum(dtype=np.uint64))
                col_file += [stems[i]] * len(names)
                col_name += names
                col_len.append(lengths)
                col_rows.append(rows)
    finally:
        hr.release_reference_dbs()
    from .engine import CLASSIFY_ROW_DTYPE

    lengths = np.concatenate(col_len) if col_len else np.zeros(0, dtype=np.int64)
    rows = np.concatenate(col_rows) if col_rows else np.zeros(0, dtype=CLASSIFY_ROW_DTYPE)
    logger.info(f"Classified {rows.size} records with {n_kept} kept hashes in {n_chunks} chunks ({'loop' if loop else 'device'} route).")
    with phases.phase("write_results"):
        status = status_of(rows, args.min_hits)
        write_outputs(results_folder, records_frame(col_file, col_name, lengths, rows, status, node_lineages),
                      *summary_tables(parent, node_lineages, lengths, rows, status))
