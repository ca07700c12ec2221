"""`yacht sketch sample` streamed (no GPU): the accumulator's eight entries in the header, the ctypes table and the shared
object; sketch.iter_sequence_chunks against sketch.read_sequences on every kind of input the latter accepts; the reader
thread's bounded queue; the command's parser and its switch."""
import argparse
import ctypes as C
import gzip
import os
import queue
import re

import pytest

from yacht_amd import _lib, sketch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["yh_sketch_acc_create", "yh_sketch_acc_destroy", "yh_sketch_acc_add", "yh_sketch_acc_add_device",
           "yh_sketch_acc_add_hashes", "yh_sketch_acc_get_info", "yh_sketch_acc_finish", "yh_sketch_acc_finish_device"]
INFO_FIELDS = ["n_bytes", "n_kept", "n_entries", "n_compacted", "capacity", "n_compactions", "n_rehashed_chunks"]
BUDGETS = [1, 7, 64, 1 << 30]


# ---- symbols ---------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_eight_entries():
    with open(os.path.join(ROOT, "include", "yacht_hip.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, code), name
    assert "#define YH_ABI_VERSION 8" in text and "typedef struct yh_sketch_acc yh_sketch_acc;" in code
    m = re.search(r"typedef struct yh_sketch_acc_info \{(.*?)\} yh_sketch_acc_info;", code, flags=re.S)
    assert m and [w.strip() for w in m.group(1).replace("uint64_t", "").rstrip("; \n").split(",")] == INFO_FIELDS
    assert "chunking invariance" in text  # the contract, stated where the entries are declared
    assert [len(_lib.SIGNATURES[name][1]) for name in ENTRIES] == [6, 1, 3, 3, 4, 2, 5, 4]
    assert [f for f, _t in _lib.SketchAccInfo._fields_] == INFO_FIELDS and C.sizeof(_lib.SketchAccInfo) == 56
    lib = _lib.load()
    assert lib.yh_abi_version() == 8 and all(hasattr(lib, name) for name in ENTRIES)


def test_null_handle_and_null_out_are_refused():
    lib = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    n = C.c_uint64(7)
    assert lib.yh_sketch_acc_create(0, 31, 42, 1 << 60, 0, None) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()
    assert lib.yh_sketch_acc_add(None, p, 8) == _lib.YH_ERR_INVALID_ARG
    assert b"null yh_sketch_acc handle" in lib.yh_last_error()
    assert lib.yh_sketch_acc_add_device(None, p, 8) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_sketch_acc_add_hashes(None, p, None, 1) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_sketch_acc_get_info(None, C.byref(_lib.SketchAccInfo())) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_sketch_acc_finish(None, 0, None, None, C.byref(n)) == _lib.YH_ERR_INVALID_ARG and n.value == 7
    m, a = C.c_void_p(), C.c_void_p()
    assert lib.yh_sketch_acc_finish_device(None, C.byref(m), C.byref(a), C.byref(n)) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_sketch_acc_destroy(None) == _lib.YH_OK  # (as yh_db_destroy)
    h = C.c_void_p()
    for k in (0, 256):  # ksize is checked before a device is looked for
        assert lib.yh_sketch_acc_create(0, k, 42, 1 << 60, 0, C.byref(h)) == _lib.YH_ERR_INVALID_ARG and not h
        assert b"ksize must be in [1, 255]" in lib.yh_last_error()


# ---- the reader --------------------------------------------------------------------------------------------------------------
FASTA_MULTI = b">a desc\nACGTACGT\nGGCC\n>b\nTTTT\nAAAACCCC\nG\n>empty\n>c\nACGT\n"
FASTQ = b"".join(b"@r%d x\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate([b"ACGTACGTAA", b"GG", b"TTTTTTTTTTTTTTTTTTTTTTT", b"", b"CATG"]))
LONG = b"ACGT" * 40  # a record longer than every small budget

INPUTS = {
    "fasta-multiline.fa": FASTA_MULTI,
    "fastq.fq": FASTQ,
    "fasta.fa.gz": FASTA_MULTI,
    "fastq.fq.gz": FASTQ,
    "fasta-crlf.fa": FASTA_MULTI.replace(b"\n", b"\r\n"),
    "fastq-crlf.fq": FASTQ.replace(b"\n", b"\r\n"),
    "fasta-blank-lines.fa": b"\n>a\nACGT\n\n\nGG\n   \n>b\n\nTT\n\n",
    "fasta-text-before-header.fa": b"ACGT\nGG\n>a\nTTTT\n",
    "fasta-no-header.fa": b"ACGT\nGG\n",
    "fasta-no-trailing-newline.fa": b">a\nACGT\nGGA",
    "fasta-header-last.fa": b">a\nACGT\n>b",
    "fastq-no-trailing-newline.fq": b"@r0\nACGT\n+\nIIII\n@r1\nGGCC\n+\nIIII",
    "fastq-ends-in-sequence.fq": b"@r0\nACGT\n+\nIIII\n@r1\nGGCC",
    "fastq-ends-in-header.fq": b"@r0\nACGT\n+\nIIII\n@r1",
    "fastq-header-only-newline.fq": b"@r0\n",
    "fastq-spaces.fq": b"@r0\n  ACGT \t\n+\nIIII\n",
    "empty.fq": b"",
    "empty.fa.gz": b"",
    "fastq-group-without-at.fq": b"@r0\nACGT\n+\nIIII\nr1\nGGGG\n+\nIIII\n@r2\nTTTT\n+\nIIII\n",
    "fastq-quality-starts-with-at.fq": b"@r0\nACGT\n+\n@III\n@r1\nCCCC\n+\n@@@@\n",
    "fasta-long-record.fa": b">s\nAC\n>l\n" + LONG[:80] + b"\n" + LONG[80:] + b"\n>t\nGT\n",
    "fastq-long-record.fq": b"@s\nAC\n+\nII\n@l\n" + LONG + b"\n+\n" + b"I" * len(LONG) + b"\n@t\nGT\n+\nII\n",
    "one-line-no-newline.fa": b">only",
}


@pytest.fixture(scope="module")
def input_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads")
    paths = {}
    for name, data in INPUTS.items():
        p = d / name
        if name.endswith(".gz"):
            with gzip.open(p, "wb") as f:
                f.write(data)
        else:
            p.write_bytes(data)
        paths[name] = str(p)
    return paths


def _sequences_of(chunks):
    return [s for c in chunks for s in c.split(b"\n")]


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_chunks_hold_the_sequences_of_read_sequences(input_files, name, budget):
    want = [s for _n, s in sketch.read_sequences(input_files[name])]
    # (block sizes: the default, which takes every file here in one read, and small ones that cut lines and records)
    for block in (sketch.READ_BLOCK_BYTES, 1, 5, 64):
        chunks = list(sketch.iter_sequence_chunks(input_files[name], budget, block_bytes=block))
        assert all(isinstance(c, bytes) for c in chunks)
        assert _sequences_of(chunks) == want, (name, budget, block)
        longest = max([len(s) for s in want], default=0)
        assert all(len(c) <= max(budget, longest) + 1 for c in chunks), (name, budget, block)
        if budget == 1:
            assert len(chunks) == len(want)      # every record alone
        if budget == 1 << 30:
            assert len(chunks) == (1 if want else 0)


def test_the_inputs_cover_what_they_claim(input_files):
    seqs = {n: [s for _n, s in sketch.read_sequences(p)] for n, p in input_files.items()}
    assert seqs["fasta-multiline.fa"] == [b"ACGTACGTGGCC", b"TTTTAAAACCCCG", b"", b"ACGT"]
    assert seqs["fasta.fa.gz"] == seqs["fasta-multiline.fa"] == seqs["fasta-crlf.fa"]
    assert seqs["fastq.fq"] == seqs["fastq.fq.gz"] == seqs["fastq-crlf.fq"] and len(seqs["fastq.fq"]) == 5
    assert seqs["fasta-blank-lines.fa"] == [b"ACGTGG", b"TT"]
    assert seqs["fasta-no-trailing-newline.fa"] == [b"ACGTGGA"] and seqs["fastq-ends-in-sequence.fq"] == [b"ACGT", b"GGCC"]
    assert seqs["fastq-ends-in-header.fq"] == [b"ACGT"] and seqs["fastq-header-only-newline.fq"] == [b""]
    assert seqs["fastq-group-without-at.fq"] == [b"ACGT", b"TTTT"]
    assert seqs["empty.fq"] == [] and seqs["empty.fa.gz"] == [] and seqs["fasta-no-header.fa"] == []
    assert max(len(s) for s in seqs["fasta-long-record.fa"]) == len(LONG) > max(BUDGETS[:3])
    assert seqs["fastq-long-record.fq"] == [b"AC", LONG, b"GT"]


def test_a_chunk_is_filled_up_to_the_budget(tmp_path):
    p = tmp_path / "r.fq"
    p.write_bytes(b"".join(b"@r\n%s\n+\n%s\n" % (b"ACGTA", b"IIIII") for _ in range(10)))
    for block in (sketch.READ_BLOCK_BYTES, 16):
        chunks = list(sketch.iter_sequence_chunks(str(p), 17, block_bytes=block))  # three records and two newlines
        assert [len(c) for c in chunks] == [17, 17, 17, 5]


def test_reader_thread_stays_two_chunks_ahead(input_files, monkeypatch):
    made = []

    class Watched(queue.Queue):
        def __init__(self, maxsize=0):
            super().__init__(maxsize)
            self.deepest = 0
            made.append(self)

        def _put(self, item):  # (called with the queue's lock held, behind its "not full" wait)
            super()._put(item)
            self.deepest = max(self.deepest, self._qsize())

    monkeypatch.setattr(sketch, "_ChunkQueue", Watched)
    paths = [input_files["fastq.fq.gz"], input_files["fasta-multiline.fa"], input_files["empty.fq"]]
    want = [s for p in paths for _n, s in sketch.read_sequences(p)]
    got = list(sketch.read_chunks_ahead(paths, 1))
    assert got == want and len(got) > 4
    assert len(made) == 1 and made[0].maxsize == sketch.READ_AHEAD_CHUNKS == 2 and 1 <= made[0].deepest <= 2
    # a consumer that stops early leaves no thread behind, and a reader's error reaches the consumer
    it = sketch.read_chunks_ahead(paths, 1)
    assert next(it) == want[0]
    it.close()
    with pytest.raises(FileNotFoundError):
        list(sketch.read_chunks_ahead([input_files["fastq.fq"], str(input_files["fastq.fq"]) + ".missing"], 1 << 20))
    import threading
    assert not [t for t in threading.enumerate() if t.name == "yacht-sketch-reader"]


# ---- the command -----------------------------------------------------------------------------------------------------------
def test_parser_is_unchanged_and_the_switch_is_read(monkeypatch):
    ap = argparse.ArgumentParser()
    sketch.add_sample_arguments(ap)
    args = ap.parse_args(["--infile", "a.fq", "b.fq", "--outfile", "o.zip"])
    assert vars(args) == {"infile": ["a.fq", "b.fq"], "kmer": 31, "scaled": 1000, "outfile": "o.zip"}
    monkeypatch.delenv("YACHT_SKETCH_SAMPLE", raising=False)
    assert sketch.use_whole_sample_path() is False
    monkeypatch.setenv("YACHT_SKETCH_SAMPLE", "whole")
    assert sketch.use_whole_sample_path() is True
    monkeypatch.setenv("YACHT_SKETCH_SAMPLE", "stream")
    assert sketch.use_whole_sample_path() is False
    monkeypatch.delenv("YACHT_SKETCH_BATCH_BYTES", raising=False)
    assert sketch.batch_bytes() == sketch.DEFAULT_BATCH_BYTES == 256 << 20
    monkeypatch.setenv("YACHT_SKETCH_BATCH_BYTES", "4096")
    assert sketch.batch_bytes() == 4096
    # the one-or-two-files check comes first on both paths, with the same message
    for mode in ("whole", ""):
        monkeypatch.setenv("YACHT_SKETCH_SAMPLE", mode)
        for files in ([], ["a", "b", "c"]):
            with pytest.raises(ValueError, match="either one file for single-end reads or two files for paired-end reads"):
                sketch.main_sample(argparse.Namespace(infile=files, kmer=31, scaled=1000, outfile="o.zip"))
