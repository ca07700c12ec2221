"""`yacht classify` without a device: the refusals and their texts, the status rule, the summary's sums, and the record reader
against sketch.read_sequences."""
import argparse
import gzip
import json
import os

import numpy as np
import pytest

from yacht_amd import classify, cli, sketch
from yacht_amd.engine import CLASSIFY_ROW_DTYPE

NONE = 0xFFFFFFFF


def _args(tmp_path, **kw):
    cfg = tmp_path / "db_config.json"
    man = tmp_path / "manifest.tsv"
    lin = tmp_path / "lineages.csv"
    fa = tmp_path / "contigs.fa"
    if not cfg.exists():
        man.write_text("organism_name\tmd5sum\n")
        cfg.write_text(json.dumps({"manifest_file_path": str(man), "intermediate_files_dir": str(tmp_path), "scale": 1000, "ksize": 31}))
        lin.write_text("ident,superkingdom\n")
        fa.write_text(">a\nACGT\n")
    base = dict(json=str(cfg), lineages=str(lin), infile=[str(fa)], outdir=str(tmp_path / "out"), min_hits=2, num_threads=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_every_refusal_comes_before_any_work(tmp_path, monkeypatch):
    monkeypatch.delenv(classify.ROUTE_ENV, raising=False)
    ok = _args(tmp_path)
    assert classify.check_options(ok) == ([ok.infile[0]], False)
    cases = [
        (dict(json=str(tmp_path / "nope.json")), FileNotFoundError, classify.MSG_NO_CONFIG.format(str(tmp_path / "nope.json"))),
        (dict(lineages=str(tmp_path / "nope.csv")), FileNotFoundError, classify.MSG_NO_LINEAGES.format(str(tmp_path / "nope.csv"))),
        (dict(min_hits=0), ValueError, classify.MSG_MIN_HITS.format(0)),
        (dict(min_hits=-3), ValueError, classify.MSG_MIN_HITS.format(-3)),
        (dict(infile=None), ValueError, classify.MSG_NO_INFILE),
        (dict(infile=[]), ValueError, classify.MSG_NO_INFILE),
        (dict(infile=[ok.infile[0], str(tmp_path / "sub" / "contigs.fasta.gz")]), ValueError,
         classify.MSG_SAME_STEM.format(ok.infile[0], str(tmp_path / "sub" / "contigs.fasta.gz"), "contigs")),
        (dict(infile=[str(tmp_path / "absent.fa")]), FileNotFoundError, classify.MSG_NO_INPUT_FILE.format(str(tmp_path / "absent.fa"))),
    ]
    for kw, exc, text in cases:
        with pytest.raises(exc) as e:
            classify.main(_args(tmp_path, **kw))
        assert str(e.value) == text, kw
    os.remove(tmp_path / "manifest.tsv")
    with pytest.raises(FileNotFoundError) as e:
        classify.main(ok)
    assert str(e.value) == classify.MSG_NO_MANIFEST.format(str(tmp_path / "manifest.tsv"))
    (tmp_path / "manifest.tsv").write_text("organism_name\tmd5sum\n")
    monkeypatch.setenv(classify.ROUTE_ENV, "fast")
    with pytest.raises(ValueError) as e:
        classify.main(ok)
    assert str(e.value) == classify.MSG_BAD_ROUTE.format("fast")
    monkeypatch.setenv(classify.ROUTE_ENV, "loop")
    assert classify.check_options(ok) == ([ok.infile[0]], True)
    assert not (tmp_path / "out").exists()  # nothing was written by any of them


def test_the_command_is_registered(tmp_path):
    args = cli.build_parser().parse_args(["classify", "--json", "c.json", "--lineages", "l.csv", "--infile", "a.fa", "b.fq.gz", "--outdir", "o"])
    assert args.func is classify.main and args.min_hits == 2 and args.infile == ["a.fa", "b.fq.gz"] and args.num_threads == 16
    assert cli.build_parser().parse_args(["classify", "--json", "c", "--lineages", "l"]).infile is None  # refused by main, with its text
    assert classify.file_stem("/x/y/reads.fastq.gz") == "reads" and classify.file_stem("bins.fa") == "bins"


def _rows(table):
    return np.array(table, dtype=CLASSIFY_ROW_DTYPE)


def test_status_rule_and_the_boundaries_of_min_hits():
    #                 node  kept hit root
    rows = _rows([(NONE, 0, 0, 0),     # no_hashes
                  (NONE, 7, 0, 0),     # not_in_database
                  (0, 7, 3, 3),        # uninformative: root hits only
                  (5, 9, 1, 0),        # i = 1
                  (5, 9, 4, 3),        # i = 1 beside three root hits
                  (5, 9, 2, 0),        # i = 2
                  (0, 9, 2, 0),        # i = 2, the fold is the root
                  (5, 9, 3, 0),        # i = 3
                  (0, 9, 5, 2)])       # i = 3, the fold is the root
    S = classify
    assert classify.status_of(rows, 1).tolist() == [S.NO_HASHES, S.NOT_IN_DATABASE, S.UNINFORMATIVE, S.CLASSIFIED, S.CLASSIFIED,
                                                    S.CLASSIFIED, S.CONFLICT, S.CLASSIFIED, S.CONFLICT]
    assert classify.status_of(rows, 2).tolist() == [S.NO_HASHES, S.NOT_IN_DATABASE, S.UNINFORMATIVE, S.BELOW_MIN_HITS, S.BELOW_MIN_HITS,
                                                    S.CLASSIFIED, S.CONFLICT, S.CLASSIFIED, S.CONFLICT]
    assert classify.status_of(rows, 3).tolist() == [S.NO_HASHES, S.NOT_IN_DATABASE, S.UNINFORMATIVE, S.BELOW_MIN_HITS, S.BELOW_MIN_HITS,
                                                    S.BELOW_MIN_HITS, S.BELOW_MIN_HITS, S.CLASSIFIED, S.CONFLICT]
    assert classify.status_of(rows, 4).tolist()[3:] == [S.BELOW_MIN_HITS] * 6
    assert classify.status_of(_rows([]), 2).size == 0


def test_summary_sums_and_the_record_table(tmp_path):
    # root 0; A 1, B 2; A;g 3 (in 1), A;h 4 (in 1); A;g;s 5 (in 3)
    parent = np.array([0, 0, 0, 1, 1, 3], dtype=np.uint32)
    lineages = [(), ("A",), ("B",), ("A", "g"), ("A", "h"), ("A", "g", "s")]
    rows = _rows([(5, 10, 4, 0), (5, 10, 4, 1), (3, 10, 2, 0), (4, 3, 3, 0), (2, 5, 5, 0), (1, 8, 6, 0), (0, 9, 4, 0), (NONE, 4, 0, 0),
                  (NONE, 0, 0, 0), (0, 6, 2, 2), (4, 6, 1, 0)])
    lengths = np.array([1000, 2000, 300, 40, 50, 600, 7000, 80, 9, 100, 110])
    status = classify.status_of(rows, 2)
    stat, tax = classify.summary_tables(parent, lineages, lengths, rows, status)
    assert stat.values.tolist() == [["no_hashes", 1, 9], ["not_in_database", 1, 80], ["uninformative", 1, 100], ["below_min_hits", 1, 110],
                                    ["conflict", 1, 7000]]
    assert list(tax.columns) == classify.SUMMARY_COLUMNS
    assert tax[["rank", "lineage", "n_records_direct", "n_records_clade", "bases_direct", "bases_clade"]].values.tolist() == [
        ["root", "", 0, 6, 0, 3990], ["superkingdom", "A", 1, 5, 600, 3940], ["phylum", "A;g", 1, 3, 300, 3300],
        ["class", "A;g;s", 2, 2, 3000, 3000], ["phylum", "A;h", 1, 1, 40, 40], ["superkingdom", "B", 1, 1, 50, 50]]
    assert tax["f_records_clade"].tolist() == [c / 11 for c in (6, 5, 3, 2, 1, 1)]
    assert tax["f_bases_clade"].tolist() == [b / int(lengths.sum()) for b in (3990, 3940, 3300, 3000, 40, 50)]
    # status rows + the root's clade = the input
    assert stat["n_records"].sum() + tax["n_records_clade"][0] == rows.size
    assert stat["bases"].sum() + tax["bases_clade"][0] == lengths.sum()
    names = [f"r{i} some text" for i in range(rows.size)]
    rec = classify.records_frame(["f"] * rows.size, names, lengths, rows, status, lineages)
    assert list(rec.columns) == classify.RECORD_COLUMNS
    assert rec["record"].tolist() == [f"r{i}" for i in range(rows.size)]
    assert rec.loc[0].tolist() == ["f", "r0", 1000, 10, 4, 0, "classified", "class", "A;g;s"]
    assert rec.loc[6].tolist() == ["f", "r6", 7000, 9, 4, 0, "conflict", "", ""]
    assert rec.loc[10].tolist() == ["f", "r10", 110, 6, 1, 0, "below_min_hits", "", ""]
    classify.write_outputs(str(tmp_path), rec, stat, tax)
    lines = (tmp_path / classify.SUMMARY_NAME).read_text().split("\n")
    assert lines[0] == "\t".join(classify.STATUS_COLUMNS) and lines[6] == "\t".join(classify.SUMMARY_COLUMNS) and lines[7].startswith("root\t\t0\t6\t")
    assert (tmp_path / classify.RECORDS_NAME).read_text().split("\n")[1] == "f\tr0\t1000\t10\t4\t0\tclassified\tclass\tA;g;s"
    # nothing classified: the root row is there, with zeros
    none = classify.status_of(rows, 100)
    stat0, tax0 = classify.summary_tables(parent, lineages, lengths, rows, none)
    assert tax0.values.tolist() == [["root", "", 0, 0, 0, 0, 0.0, 0.0]] and stat0["n_records"].sum() == rows.size


FASTA = (b"junk before the first header\n>one first record\nACGT\nAC\n\n>two\n>three  \nGGGG   \n\n>four\nTT")
FASTQ = (b"@r1 x\nACGT\n+\nIIII\n@r2\n\n+\n\n@r3\n  GGCC  \n+r3\nIIII\nnot a header\nAAAA\n+\nIIII\n@r5\nTTTT")
CRLF = b">c1 desc\r\nACGT\r\nGG\r\n>c2\r\n\r\n>c3\r\nTTTT\r\n"
CRLF_Q = b"@q1\r\nACGT\r\n+\r\nIIII\r\n@q2\r\nGG\r\n+\r\nII\r\n"


@pytest.mark.parametrize("name,data", [("a.fa", FASTA), ("a.fq", FASTQ), ("a.fa.gz", FASTA), ("a.fq.gz", FASTQ), ("crlf.fa", CRLF),
                                       ("crlf.fq", CRLF_Q), ("empty.fa", b""), ("hdr.fq", b"@only\n"), ("nl.fa", b"\n>x\nAC\n"),
                                       ("last.fq", b"@a\nAC\n+\nII\n@b")])
def test_record_reader_equals_read_sequences(tmp_path, name, data):
    path = tmp_path / name
    if name.endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        path.write_bytes(data)
    want = list(sketch.read_sequences(str(path)))
    assert list(classify.iter_records(str(path))) == want
    if name in ("a.fa", "a.fq"):
        assert len(want) == 4 and want[1][1] == b""  # (the cases hold what they are meant to hold)
    total = sum(len(s) for _n, s in want)
    longest = max([len(s) for _n, s in want] + [0])
    for budget in (1, max(longest, 1), total + 10):
        chunks = list(classify.iter_record_chunks(str(path), budget))
        names = [n for c in chunks for n in c[0]]
        assert names == [n for n, _s in want]
        seqs = []
        for c_names, lengths, buf, off in chunks:
            assert buf.dtype == np.uint8 and off.dtype == np.uint64 and off[0] == 0 and int(off[-1]) == buf.size
            assert lengths.tolist() == np.diff(off.astype(np.int64)).tolist() and len(c_names) == lengths.size >= 1
            assert buf.size <= budget or lengths.size == 1
            seqs += [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(lengths.size)]
        assert seqs == [s for _n, s in want]
        if budget == 1:
            assert len(chunks) == len(want) or any(len(s) == 0 for _n, s in want)
        if budget > total and want:
            assert len(chunks) == 1
    ahead = list(classify.read_record_chunks_ahead([str(path), str(path)], 1))
    assert [i for i, *_ in ahead] == sorted(i for i, *_ in ahead) and [n for _i, ns, *_ in ahead for n in ns] == [n for n, _s in want] * 2


def test_crlf_names_and_sequences(tmp_path):
    path = tmp_path / "crlf.fa"
    path.write_bytes(CRLF)
    (names, lengths, buf, off), = classify.iter_record_chunks(str(path), 1 << 20)
    assert [n.split()[0] for n in names] == ["c1", "c2", "c3"] and lengths.tolist() == [6, 0, 4] and buf.tobytes() == b"ACGTGGTTTT"


def test_reader_errors_reach_the_consumer(tmp_path):
    with pytest.raises(FileNotFoundError):
        list(classify.read_record_chunks_ahead([str(tmp_path / "absent.fa")], 10))
