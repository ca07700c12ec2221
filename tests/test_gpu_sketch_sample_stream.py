"""`yacht sketch sample` streamed through the device accumulator against the path that reads every file whole
(YACHT_SKETCH_SAMPLE=whole): the same .sig.zip, member for member -- signature name, filename, mins, abundances, md5 and the
manifest -- whatever the chunk budget (YACHT_SKETCH_BATCH_BYTES)."""
import gzip
import json
import os
import zipfile

import numpy as np
import pytest

from oracle import sketch_oracle as so

pytestmark = pytest.mark.gpu
FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")


def _members(path):
    """{member name: its content} with every signature member gunzipped and parsed"""
    out = {}
    with zipfile.ZipFile(path) as z:
        for name in z.namelist():
            raw = z.read(name)
            out[name] = json.loads(gzip.decompress(raw)) if name.endswith(".sig.gz") else raw.decode("utf-8").splitlines()
        return z.namelist(), out


@pytest.fixture(scope="module")
def read_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sample")
    seq = b"".join(s for _n, s in list(so.read_fasta(os.path.join(FX, "GCF_018918045.1_genomic.fna.gz")))[:3])[:60000]
    reads = [seq[i:i + 120] for i in range(0, len(seq) - 120, 60)]
    reads += reads[::7]                      # some reads twice
    paths = []
    for tag, part in (("R1", reads[::2]), ("R2", reads[1::2])):
        p = d / f"{tag}.fq.gz"
        with gzip.open(p, "wb") as f:
            for i, r in enumerate(part):
                f.write(b"@%s.%d\n" % (tag.encode(), i) + r + b"\n+\n" + b"I" * len(r) + b"\n")
        paths.append(str(p))
    fa = d / "contigs.fa"
    fa.write_bytes(b"".join(b">c%d\n" % j + b"\n".join(seq[o:o + 7000][i:i + 70] for i in range(0, 7000, 70)) + b"\n"
                            for j, o in enumerate((1000, 5000, 41000))))   # (the first two overlap: counts of 2)
    paths.append(str(fa))
    return paths, reads


def _run(monkeypatch, infiles, out, batch_bytes=None, whole=False):
    from yacht_amd import cli

    monkeypatch.delenv("YACHT_SKETCH_SAMPLE", raising=False)
    monkeypatch.delenv("YACHT_SKETCH_BATCH_BYTES", raising=False)
    if batch_bytes is not None:
        monkeypatch.setenv("YACHT_SKETCH_BATCH_BYTES", str(batch_bytes))
    if whole:
        monkeypatch.setenv("YACHT_SKETCH_SAMPLE", "whole")
    assert cli.main(["sketch", "sample", "--infile", *infiles, "--scaled", "10", "--outfile", str(out)]) == 0
    return _members(str(out))


@pytest.mark.parametrize("which", ["two-fastq-gz", "one-fasta"])
def test_three_runs_write_the_same_archive(hip_lib, read_files, tmp_path, monkeypatch, which):
    from yacht_amd import sigio

    paths, reads = read_files
    infiles = paths[:2] if which == "two-fastq-gz" else paths[2:]
    small = _run(monkeypatch, infiles, tmp_path / "small.sig.zip", batch_bytes=4096)
    default = _run(monkeypatch, infiles, tmp_path / "default.sig.zip")
    whole = _run(monkeypatch, infiles, tmp_path / "whole.sig.zip", whole=True)
    assert small[0] == default[0] == whole[0] and len(whole[0]) == 2      # member names, in order
    assert small[1] == default[1] == whole[1]                              # signature JSON and manifest rows
    (sig_name,) = [n for n in whole[0] if n.endswith(".sig.gz")]
    (rec,) = whole[1][sig_name]
    (s,) = rec["signatures"]
    assert rec["name"] == os.path.basename(infiles[0]) and rec["filename"] == infiles[0]
    assert s["md5sum"] == sigio.md5_of_mins(31, s["mins"]) and sig_name == f"signatures/{s['md5sum']}.sig.gz"
    assert len(s["mins"]) == len(s["abundances"]) > 1000 and max(s["abundances"]) >= 2
    if which == "two-fastq-gz":      # ... and they are right
        m, a = so.sketch_records(reads, 31, 10)
        assert np.array_equal(np.array(s["mins"], dtype=np.uint64), m) and np.array_equal(np.array(s["abundances"]), a)


def test_file_count_is_checked_on_both_paths(hip_lib, read_files, tmp_path, monkeypatch):
    from yacht_amd import cli

    paths, _ = read_files
    for mode in ("", "whole"):
        monkeypatch.setenv("YACHT_SKETCH_SAMPLE", mode)
        with pytest.raises(ValueError, match="either one file for single-end reads or two files for paired-end reads"):
            cli.main(["sketch", "sample", "--infile", *paths, "--outfile", str(tmp_path / "x.sig.zip")])
        assert not (tmp_path / "x.sig.zip").exists()
