"""`yacht run` with several --sample_file values (yacht_amd/cohort.py): the command line and the checks made before any
device work.  No GPU: every case here ends in a check, with nothing written and no database built."""
import json
import os
import shutil
import zipfile

import numpy as np
import pytest

from yacht_amd import cli, cohort, run_YACHT, sigio

FX = os.path.join(os.path.dirname(__file__), "golden", "fixtures")


@pytest.fixture
def setup(tmp_path, monkeypatch):
    """A config + manifest as `yacht train` leaves them, an output directory, and a guard that fails on device work."""
    work = tmp_path / "db_intermediate_files"
    work.mkdir()
    manifest = tmp_path / "db_processed_manifest.tsv"
    manifest.write_text("organism_name\tmd5sum\tnum_unique_kmers_in_genome_sketch\tnum_total_kmers_in_genome_sketch\t"
                        "genome_scale_factor\norg\t0123\t10\t10\t1000\n")
    cfg = tmp_path / "db_config.json"
    cfg.write_text(json.dumps({"manifest_file_path": str(manifest), "intermediate_files_dir": str(work), "scale": 1000,
                               "ksize": 31, "ani_thresh": 0.95}))
    out = tmp_path / "out"
    out.mkdir()

    def no_device(*a, **k):
        raise AssertionError("device work started before every input was checked")

    monkeypatch.setattr(cohort.hr, "get_reference_db", no_device)
    monkeypatch.setattr(cohort, "_Device", no_device)
    return tmp_path, cfg, out


def _run(cfg, out, files):
    return cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(out)])


def _sample(path, n=200, scaled=1000, seed=0):
    rng = np.random.default_rng(seed)
    mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(scaled), n, dtype=np.uint64))
    sigio.write_sig_zip([sigio.make_signature(mins, ksize=31, scaled=scaled, name=os.path.basename(str(path)),
                                              abundances=np.ones(mins.size, dtype=np.int64))], str(path))
    return path


def test_parser_takes_several_sample_files():
    args = cli.build_parser().parse_args(["run", "--json", "c.json", "--sample_file", "a.sig.zip", "b.sig.zip", "c.sig.zip"])
    assert args.sample_file == ["a.sig.zip", "b.sig.zip", "c.sig.zip"]
    one = cli.build_parser().parse_args(["run", "--json", "c.json", "--sample_file", "a.sig.zip"])
    assert one.sample_file == ["a.sig.zip"] and one.func is run_YACHT.main


def test_duplicate_stems_rejected(setup):
    tmp, cfg, out = setup
    (tmp / "x").mkdir()
    (tmp / "y").mkdir()
    a = _sample(tmp / "x" / "s1.sig.zip")
    b = _sample(tmp / "y" / "s1.sig.zip", seed=1)
    c = _sample(tmp / "s2.sig.zip", seed=2)
    with pytest.raises(ValueError, match=r"share the name 's1'") as ei:
        _run(cfg, out, [c, a, b])
    assert str(b) in str(ei.value)
    assert not (out / "results").exists()


def test_bad_scale_names_the_file(setup):
    tmp, cfg, out = setup
    good = _sample(tmp / "good.sig.zip")
    bad = _sample(tmp / "bad.sig.zip", scaled=2000)
    with pytest.raises(ValueError, match=run_YACHT.MSG_SCALE_MISMATCH) as ei:
        _run(cfg, out, [good, bad])
    assert str(bad) in str(ei.value)
    assert not (out / "results").exists()


def test_archive_without_manifest_names_the_file(setup):
    tmp, cfg, out = setup
    good = _sample(tmp / "good.sig.zip")
    src = _sample(tmp / "src.sig.zip", seed=3)
    bare = tmp / "bare.sig.zip"
    with zipfile.ZipFile(src) as zi, zipfile.ZipFile(bare, "w") as zo:
        for name in zi.namelist():
            if name != "SOURMASH-MANIFEST.csv":
                zo.writestr(name, zi.read(name))
    os.remove(src)
    with pytest.raises(FileNotFoundError) as ei:
        _run(cfg, out, [good, bare])
    assert str(ei.value) == run_YACHT.MSG_ZIP_WITHOUT_MANIFEST.format(str(bare))
    assert not (out / "results").exists()


def test_wrong_ksize_names_the_file(setup):
    tmp, cfg, out = setup
    good = _sample(tmp / "good.sig.zip")
    other = tmp / "k21.sig.zip"
    rng = np.random.default_rng(5)
    mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 100, dtype=np.uint64))
    sigio.write_sig_zip([sigio.make_signature(mins, ksize=21, scaled=1000)], str(other))
    with pytest.raises(ValueError) as ei:
        _run(cfg, out, [good, other])
    assert str(ei.value) == run_YACHT.MSG_NOT_ONE_SKETCH.format(str(other), 31, len(str(other)))
    assert not (out / "results").exists()


def test_fixture_sample_passes_the_checks(setup, tmp_path):
    """The checks accept real sourmash archives (the fixture sample under two names) and stop at the device guard."""
    tmp, cfg, out = setup
    a, b = tmp / "a.sig.zip", tmp / "b.sig.zip"
    shutil.copyfile(os.path.join(FX, "sample.sig.zip"), a)
    shutil.copyfile(os.path.join(FX, "sample.sig.zip"), b)
    plan = cohort.check_inputs(cli.build_parser().parse_args(["run", "--json", str(cfg), "--sample_file", str(a), str(b),
                                                               "--outdir", str(out)]), [str(a), str(b)])
    assert [m[2] for m in plan["meta"]] == [1000, 1000]  # (n_hashes, mean_abundance, scaled): no sketch kept
    assert plan["meta"][0] == plan["meta"][1] and plan["meta"][0][0] > 0
    with pytest.raises(AssertionError, match="device work"):
        _run(cfg, out, [a, b])


def test_block_constants_follow_the_header():
    """The driver's block size and coverages per launch are the header's (yacht_amd/_lib.py mirrors them)."""
    import re

    from yacht_amd import _lib

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        text = f.read()
    for name in ("YH_BATCH_MAX_SAMPLES", "YH_PRESENCE_MAX_COVS"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name)
    assert cohort.BLOCK == _lib.YH_BATCH_MAX_SAMPLES and cohort.MAX_COVS == _lib.YH_PRESENCE_MAX_COVS
