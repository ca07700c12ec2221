"""GPU: `yacht sketch ref` through the segmented sketcher (many records / files per device call) against the one-call-per-
record / per-file path it replaces (YACHT_SKETCH_REF=loop): the same signatures in the same order."""
import gzip
import os
import zipfile

import numpy as np
import pytest

import test_gpu_sketch_edges as edges
from oracle import sketch_oracle as so

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")


def _fasta(records, width=70):
    out = []
    for name, seq in records:
        out.append(b">" + name.encode() + b"\n")
        out += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
    return b"".join(out)


def _run_ref(monkeypatch, infile, outfile, kmer, scaled, env):
    from yacht_amd import cli

    for var in ("YACHT_SKETCH_REF", "YACHT_SKETCH_BATCH_BYTES"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    assert cli.main(["sketch", "ref", "--infile", str(infile), "--kmer", str(kmer), "--scaled", str(scaled), "--outfile", str(outfile)]) == 0


def _load(path, kmer):
    from yacht_amd import sigio

    sigs = sigio.load_file_as_signatures(str(path), ksize=kmer)
    with zipfile.ZipFile(path) as z:
        manifest = z.read(sigio.MANIFEST_NAME).decode()
    return sigs, manifest


def _assert_same(a, b):
    (sa, ma), (sb, mb) = a, b
    assert [s.name for s in sa] == [s.name for s in sb]
    assert [s.filename for s in sa] == [s.filename for s in sb]
    assert [s.md5sum() for s in sa] == [s.md5sum() for s in sb]
    for x, y in zip(sa, sb):
        assert np.array_equal(x.minhash.mins, y.minhash.mins), x.name
        assert np.array_equal(np.asarray(x.minhash.abundances), np.asarray(y.minhash.abundances)), x.name
    assert ma == mb     # manifest rows


def test_file_of_records(hip_lib, tmp_path, monkeypatch):
    rng = np.random.default_rng(77)
    genome = edges.random_bases(6000, 78, True)
    records = []
    for i in range(40):
        n = int(rng.integers(20, 400)) if i % 7 else 25       # (some shorter than k: empty sketches)
        s = int(rng.integers(0, genome.size - n))
        seq = genome[s:s + n].copy()
        if i % 5 == 0:
            seq[n // 2] = ord("N")
        records.append((f"rec{i} sample record", seq.tobytes()))
    twice = genome[100:400].tobytes()
    records[6] = (records[6][0], twice + b"N" + twice)        # ... and twice in one record: abundances of 2
    fa = tmp_path / "records.fa"
    fa.write_bytes(_fasta(records))
    _run_ref(monkeypatch, fa, tmp_path / "batch.sig.zip", 31, 3, {})
    _run_ref(monkeypatch, fa, tmp_path / "loop.sig.zip", 31, 3, {"YACHT_SKETCH_REF": "loop"})
    batch, loop = _load(tmp_path / "batch.sig.zip", 31), _load(tmp_path / "loop.sig.zip", 31)
    _assert_same(batch, loop)
    assert [s.name for s in batch[0]] == [n for n, _s in records] and len(batch[0]) == 40
    for (name, seq), sig in zip(records, batch[0]):          # and the oracle, record by record
        m, a = so.sketch_records([seq], 31, 3)
        assert np.array_equal(sig.minhash.mins, m) and np.array_equal(np.asarray(sig.minhash.abundances), a), name
    assert any(len(s.minhash) == 0 for s in batch[0]) and len(batch[0][6].minhash) > 0
    assert np.asarray(batch[0][6].minhash.abundances).tolist() == [2] * len(batch[0][6].minhash)


def test_folder_of_genomes(hip_lib, tmp_path, monkeypatch):
    gdir = tmp_path / "genomes"
    (gdir / "sub").mkdir(parents=True)
    a = [(f"a{i}", edges.random_bases(3000 + 17 * i, 80 + i).tobytes()) for i in range(4)]
    b = [(f"b{i}", edges.random_bases(2500, 90 + i, True).tobytes()) for i in range(3)] + [a[1]]   # shares a record with a
    (gdir / "alpha.fna").write_bytes(_fasta(a))
    with gzip.open(gdir / "sub" / "beta.fa.gz", "wb") as f:
        f.write(_fasta(b))
    (gdir / "gamma.fasta").write_bytes(_fasta([("short", b"ACGTACGTACGTAC")]))   # one record shorter than k
    (gdir / "notes.txt").write_text("not a genome")
    outs = {}
    for tag, env in (("batch", {}), ("loop", {"YACHT_SKETCH_REF": "loop"}), ("three", {"YACHT_SKETCH_BATCH_BYTES": "9000"})):
        _run_ref(monkeypatch, gdir, tmp_path / f"{tag}.sig.zip", 31, 10, env)
        outs[tag] = _load(tmp_path / f"{tag}.sig.zip", 31)
    _assert_same(outs["batch"], outs["loop"])
    _assert_same(outs["three"], outs["loop"])
    sigs = outs["batch"][0]
    assert [s.name for s in sigs] == ["alpha", "beta", "gamma"] and len(sigs[2].minhash) == 0
    for sig, recs in zip(sigs, (a, b)):
        m, c = so.sketch_records([s for _n, s in recs], 31, 10)
        assert np.array_equal(sig.minhash.mins, m) and np.array_equal(np.asarray(sig.minhash.abundances), c)
    # 9 000 bytes hold none of the pairs of files: three calls
    from yacht_amd import sketch

    sizes = [len(sketch._read_unit(str(p))[1]) for p in (gdir / "alpha.fna", gdir / "sub" / "beta.fa.gz", gdir / "gamma.fasta")]
    assert sizes[0] > 9000 and sizes[1] > 9000 and sizes[1] + sizes[2] > 9000
    calls = []
    real = sketch.sketch_segments
    monkeypatch.setattr(sketch, "sketch_segments", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    monkeypatch.setenv("YACHT_SKETCH_BATCH_BYTES", "9000")
    got = sketch.sketch_files([str(gdir / "alpha.fna"), str(gdir / "sub" / "beta.fa.gz"), str(gdir / "gamma.fasta")], str(tmp_path / "files.sig.zip"), 31, 10)
    assert len(calls) == 3 and [s.name for s in got] == ["a0", "b0", "short"]
    assert [s.md5sum() for s in got] == [s.md5sum() for s in sigs]
    calls.clear()
    monkeypatch.delenv("YACHT_SKETCH_BATCH_BYTES")
    sketch.sketch_files([str(gdir / "alpha.fna"), str(gdir / "sub" / "beta.fa.gz"), str(gdir / "gamma.fasta")], str(tmp_path / "files2.sig.zip"), 31, 10)
    assert len(calls) == 1


def test_fixture_genome_through_folder_mode(hip_lib, tmp_path, monkeypatch):
    from yacht_amd import sigio

    gdir = tmp_path / "genomes"
    gdir.mkdir()
    os.symlink(os.path.join(FX, "GCF_018918045.1_genomic.fna.gz"), gdir / "GCF_018918045.1_genomic.fna.gz")
    _run_ref(monkeypatch, gdir, tmp_path / "ref.sig.zip", 31, 1000, {})
    sigs = sigio.load_file_as_signatures(str(tmp_path / "ref.sig.zip"), ksize=31)
    assert len(sigs) == 1 and sigs[0].name == "GCF_018918045.1_genomic"
    assert (len(sigs[0].minhash), int(sigs[0].minhash.abundances.sum())) == (2452, 2453)
