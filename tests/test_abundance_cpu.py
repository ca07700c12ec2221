"""`yacht run --abundance` without a GPU: the library's new symbols and their argument handling, the command line, the
pure numpy / pandas column arithmetic (yacht_amd/abundance.py), the host-side argument checks of RefDB.abundance, and the
check that stops a sample without abundances before any device work."""
import ctypes as C
import json
import os

import numpy as np
import pandas as pd
import pytest

from yacht_amd import _lib, abundance, cli, cohort, engine, run_YACHT, sigio
from yacht_amd import hypothesis_recovery_src as hr


def test_library_exposes_the_entries_and_rejects_a_null_handle():
    lib = _lib.load()
    assert hasattr(lib, "yh_abund") and hasattr(lib, "yh_abund_device")
    assert lib.yh_abi_version() == 8
    buf = np.zeros(4, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.yh_abund(None, p, p, 0, p, p, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_abund_device(None, p, p, 0, p, p, None) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()


def test_header_declares_what_the_binding_types():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        text = f.read()
    assert "int yh_abund_device(" in text and "int yh_abund(" in text and "#define YH_ABI_VERSION 8" in text
    assert "yh_abund" in _lib.SIGNATURES and "yh_abund_device" in _lib.SIGNATURES


def test_parser_takes_the_flag_and_defaults_to_off():
    base = ["run", "--json", "c.json", "--sample_file", "a.sig.zip"]
    assert cli.build_parser().parse_args(base).abundance is False
    assert cli.build_parser().parse_args(base + ["--abundance"]).abundance is True


def _columns():
    #                 present  present  absent  no exclusive match  present
    w_overlap = np.array([40, 9, 7, 5, 12], dtype=np.uint64)
    w_match = np.array([30, 6, 4, 0, 2], dtype=np.uint64)
    med = np.array([3.0, 1.5, 2.0, 0.0, 0.5])
    n_ov = np.array([12, 6, 3, 5, 0])
    n_m = np.array([10, 4, 2, 0, 4])
    present = np.array([True, True, False, False, True])
    return abundance.abundance_columns(w_overlap, w_match, med, n_ov, n_m, present, total_abundance=200)


def test_columns_order_and_values():
    df = _columns()
    assert list(df.columns) == abundance.ABUNDANCE_COLUMNS == [
        "abund_sum_overlap", "abund_mean_overlap", "abund_sum_exclusive", "abund_mean_exclusive", "abund_median_exclusive",
        "f_weighted_overlap", "relative_abundance"]
    assert df["abund_sum_overlap"].tolist() == [40, 9, 7, 5, 12] and df["abund_sum_exclusive"].tolist() == [30, 6, 4, 0, 2]
    assert df["abund_mean_overlap"].tolist()[:4] == [40 / 12, 9 / 6, 7 / 3, 1.0]
    assert df["abund_mean_exclusive"].tolist()[:3] == [3.0, 1.5, 2.0]
    assert df["f_weighted_overlap"].tolist() == [0.2, 0.045, 0.035, 0.025, 0.06]


def test_columns_nan_rules():
    df = _columns()
    # no exclusive match: mean and median are NaN, the sums stay 0
    assert np.isnan(df["abund_mean_exclusive"][3]) and np.isnan(df["abund_median_exclusive"][3])
    assert df["abund_sum_exclusive"][3] == 0 and not np.isnan(df["abund_mean_overlap"][3])
    # no overlap count (a row a duplicate organism name pulled in): its mean is NaN
    assert np.isnan(df["abund_mean_overlap"][4])
    assert not df[["abund_sum_overlap", "abund_sum_exclusive", "f_weighted_overlap", "relative_abundance"]].isna().any().any()


def test_relative_abundance_sums_to_one_over_the_present_rows():
    df = _columns()
    rel = df["relative_abundance"].to_numpy()
    assert rel[2] == 0.0 and rel[3] == 0.0  # rows not present
    assert rel[0] == 3.0 / 5.0 and rel[1] == 1.5 / 5.0 and rel[4] == 0.5 / 5.0
    assert abs(rel.sum() - 1.0) < 1e-15
    none = abundance.abundance_columns([1], [1], [1.0], [1], [1], [False], 10)
    assert none["relative_abundance"].tolist() == [0.0]
    empty = abundance.abundance_columns([], [], [], [], [], [], 0)
    assert len(empty) == 0 and list(empty.columns) == abundance.ABUNDANCE_COLUMNS


def test_columns_follow_the_hypothesis_columns_and_feed_the_profile():
    man = pd.DataFrame({"organism_name": ["a", "b", "c"], "min_coverage": 1.0})
    cols = (np.array([True, False, True]), np.zeros(3), np.array([9, 9, 9]), np.array([9, 9, 9]), np.array([4, 0, 2]),
            np.zeros(3), np.zeros(3), np.zeros(3))
    tables = []
    for cov in (1.0, 0.5):
        frame = hr.coverage_frame(man.copy(), cols, cov)
        tables.append(abundance.append_columns(frame, [8, 0, 6], [8, 0, 6], [1.0, 0.0, 3.0], [4, 1, 2], 50))
    assert list(tables[0].columns) == ["organism_name", "min_coverage"] + hr.GIVEN_COLUMNS + abundance.ABUNDANCE_COLUMNS
    prof = abundance.profile_frame(tables[::-1], [0.5, 1.0])
    assert list(prof.columns) == abundance.PROFILE_COLUMNS
    assert prof["min_coverage"].tolist() == [1.0, 1.0, 0.5, 0.5]  # coverage descending ...
    assert prof["organism_name"].tolist() == ["c", "a", "c", "a"]  # ... then relative abundance descending
    assert prof["relative_abundance"].tolist() == [0.75, 0.25, 0.75, 0.25]
    assert prof["num_matches"].tolist() == [2, 4, 2, 4]


def test_abundance_argument_checks_need_no_database():
    sample = np.arange(1, 6, dtype=np.uint64)
    s, a = engine.check_abundances(sample, [1, 2, 3, 4, 2 ** 32 - 1])
    assert s.dtype == np.uint64 and a.dtype == np.uint32 and a.tolist() == [1, 2, 3, 4, 2 ** 32 - 1]
    db = engine.RefDB.__new__(engine.RefDB)  # no handle: the checks come before any library call
    db._h = C.c_void_p(0)
    with pytest.raises(ValueError, match="one abundance per sample hash"):
        db.abundance(sample, np.ones(4, dtype=np.int64))
    with pytest.raises(ValueError, match=r"2\*\*32 - 1"):
        db.abundance(sample, np.array([1, 1, 2 ** 32, 1, 1], dtype=np.int64))
    with pytest.raises(ValueError, match=r"2\*\*32 - 1"):
        db.abundance(sample, np.array([1, 1, -1, 1, 1], dtype=np.int64))
    with pytest.raises(ValueError, match="integers"):
        db.abundance(sample, np.ones(5, dtype=np.float64))


@pytest.fixture
def setup(tmp_path, monkeypatch):
    """A hand-written config + manifest, an output directory, and a guard that fails on device work (tests/test_cohort_cli.py)."""
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

    monkeypatch.setattr(hr, "get_reference_db", no_device)
    monkeypatch.setattr(cohort, "_Device", no_device)
    return tmp_path, cfg, out


def _sample(path, with_abundance, seed=0):
    rng = np.random.default_rng(seed)
    mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 200, dtype=np.uint64))
    ab = 1 + rng.integers(0, 5, mins.size) if with_abundance else None
    sigio.write_sig_zip([sigio.make_signature(mins, ksize=31, scaled=1000, name=os.path.basename(str(path)), abundances=ab)], str(path))
    return path


def test_sample_without_abundances_is_refused_before_device_work(setup):
    tmp, cfg, out = setup
    bare = _sample(tmp / "bare.sig.zip", with_abundance=False)
    before = sorted(p.name for p in tmp.iterdir())
    with pytest.raises(ValueError) as ei:
        cli.main(["run", "--json", str(cfg), "--sample_file", str(bare), "--outdir", str(out), "--abundance"])
    assert str(bare) in str(ei.value) and "abundance" in str(ei.value)
    assert sorted(p.name for p in tmp.iterdir()) == before
    assert sorted(p.name for p in out.iterdir()) == ["results"] and not list((out / "results").iterdir())


def test_cohort_sample_without_abundances_is_refused_before_device_work(setup):
    tmp, cfg, out = setup
    good = _sample(tmp / "good.sig.zip", with_abundance=True, seed=1)
    bare = _sample(tmp / "bare.sig.zip", with_abundance=False, seed=2)
    with pytest.raises(ValueError) as ei:
        cli.main(["run", "--json", str(cfg), "--sample_file", str(good), str(bare), "--outdir", str(out), "--abundance"])
    assert str(bare) in str(ei.value)
    assert not (out / "results").exists()
    # the same files without the flag pass every check and stop at the device guard
    with pytest.raises(AssertionError, match="device work"):
        cli.main(["run", "--json", str(cfg), "--sample_file", str(good), str(bare), "--outdir", str(out)])


def test_sample_abundances_come_in_hash_order(tmp_path):
    p = _sample(tmp_path / "s.sig.zip", with_abundance=True, seed=3)
    sig = run_YACHT.utils.load_signature_with_ksize(str(p), 31)
    want = sigio.load_file_as_signatures(str(p), ksize=31)[0].minhash
    got = abundance.sample_abundances(sig, str(p))
    assert np.array_equal(got, want.abundances) and np.array_equal(sig.minhash.mins, want.mins)
