"""`yacht run --residual` without a GPU: the library's new symbols and their argument handling, the command line and its
refusals before any device work, the host-side argument checks of RefDB.explain, and the pure numpy / pandas side
(yacht_amd/residual.py): member tables, the explained table and the residual signature."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from yacht_amd import _lib, cli, cohort, engine, residual, run_YACHT, sigio, utils
from yacht_amd import hypothesis_recovery_src as hr


def test_library_exposes_the_entries_and_rejects_a_null_handle():
    lib = _lib.load()
    assert hasattr(lib, "yh_explain") and hasattr(lib, "yh_explain_device")
    assert lib.yh_abi_version() == 8
    buf = np.zeros(16, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.yh_explain(None, p, p, 0, p, p, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_explain_device(None, p, None, 0, p, None, p) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()


def test_header_declares_what_the_binding_types():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        text = f.read()
    assert "int yh_explain_device(" in text and "int yh_explain(" in text and "#define YH_ABI_VERSION 8" in text
    assert "yh_explain / yh_explain_device" in text  # its row of the interleaving table
    assert "yh_explain" in _lib.SIGNATURES and "yh_explain_device" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["yh_explain"][1]) == 7 and len(_lib.SIGNATURES["yh_explain_device"][1]) == 7


def test_parser_takes_both_options_with_their_defaults():
    base = ["run", "--json", "c.json", "--sample_file", "a.sig.zip"]
    args = cli.build_parser().parse_args(base)
    assert args.residual is False and args.residual_coverage is None
    args = cli.build_parser().parse_args(base + ["--residual", "--residual_coverage", "0.5"])
    assert args.residual is True and args.residual_coverage == 0.5
    flags = [f for f, _ in run_YACHT.ARGUMENTS]
    assert "--residual" in flags and "--residual_coverage" in flags


def test_residual_coverage_defaults_to_the_smallest_listed_value():
    base = ["run", "--json", "c.json", "--sample_file", "a.sig.zip", "--residual"]
    assert residual.residual_coverage(cli.build_parser().parse_args(base)) == 0.01
    args = cli.build_parser().parse_args(base + ["--min_coverage_list", "0.5", "1", "0.1"])
    assert residual.residual_coverage(args) == 0.1
    args = cli.build_parser().parse_args(base + ["--min_coverage_list", "0.5", "1", "0.1", "--residual_coverage", "0.5"])
    assert residual.residual_coverage(args) == 0.5


@pytest.fixture
def setup(tmp_path, monkeypatch):
    """A hand-written config + manifest, an output directory, and a guard that fails on device work (tests/test_cohort_cli.py)."""
    work = tmp_path / "db_intermediate_files"
    work.mkdir()
    manifest = tmp_path / "db_processed_manifest.tsv"
    manifest.write_text("organism_name\tmd5sum\tnum_unique_kmers_in_genome_sketch\tnum_total_kmers_in_genome_sketch\t"
                        "genome_scale_factor\norg\tabcd\t10\t10\t1000\n")
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


def _sample(path, seed=0):
    rng = np.random.default_rng(seed)
    mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 200, dtype=np.uint64))
    sigio.write_sig_zip([sigio.make_signature(mins, ksize=31, scaled=1000, name=os.path.basename(str(path)),
                                              abundances=1 + rng.integers(0, 5, mins.size))], str(path))
    return path


@pytest.mark.parametrize("n_files", [1, 2])
def test_residual_coverage_is_checked_before_device_work(setup, n_files):
    tmp, cfg, out = setup
    files = [str(_sample(tmp / f"s{i}.sig.zip", seed=i)) for i in range(n_files)]
    base = ["run", "--json", str(cfg), "--sample_file", *files, "--outdir", str(out), "--min_coverage_list", "1", "0.5"]
    before = sorted(p.name for p in tmp.iterdir())
    with pytest.raises(ValueError, match="0.25") as ei:  # not one of the list: the message names the value
        cli.main(base + ["--residual", "--residual_coverage", "0.25"])
    assert "min_coverage_list" in str(ei.value)
    with pytest.raises(ValueError, match="--residual"):  # the option without --residual
        cli.main(base + ["--residual_coverage", "0.5"])
    assert sorted(p.name for p in tmp.iterdir()) == before and not list(out.iterdir())
    # a listed value passes every check and stops at the device guard
    with pytest.raises(AssertionError, match="device work"):
        cli.main(base + ["--residual", "--residual_coverage", "0.5"])


def test_explain_argument_checks_need_no_database():
    sample = np.arange(1, 6, dtype=np.uint64)
    m = engine.check_member([0, 1, 127], 3)
    assert m.dtype == np.uint8 and m.tolist() == [0, 1, 127]
    db = engine.RefDB.__new__(engine.RefDB)  # no handle: the checks come before any library call
    db._h = C.c_void_p(0)
    db.n_refs = 3
    with pytest.raises(ValueError, match="one byte per reference"):
        db.explain(sample, np.zeros(4, dtype=np.uint8))
    with pytest.raises(ValueError, match="bit 7"):
        db.explain(sample, np.array([0, 0x80, 0], dtype=np.uint8))
    with pytest.raises(ValueError, match="bit 7"):
        db.explain(sample, np.array([0, -1, 0], dtype=np.int64))
    with pytest.raises(ValueError, match="integers"):
        db.explain(sample, np.zeros(3, dtype=np.float64))
    with pytest.raises(ValueError, match="one abundance per sample hash"):
        db.explain(sample, np.zeros(3, dtype=np.uint8), abund=np.ones(4, dtype=np.int64))
    with pytest.raises(ValueError, match=r"2\*\*32 - 1"):
        db.explain(sample, np.zeros(3, dtype=np.uint8), abund=np.array([1, 1, 2 ** 32, 1, 1], dtype=np.int64))


def test_member_table_bit_placement_and_more_than_seven_call_sets():
    sets = [[0], [0, 1], [], [2, 3], [4], [1, 4], [3]]
    t = residual.member_table(5, sets)
    assert t.dtype == np.uint8 and t.tolist() == [0b0000011, 0b0100010, 0b0001000, 0b1001000, 0b0110000]
    assert residual.member_table(3, []).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="at most 7"):
        residual.member_table(5, sets + [[0]])
    with pytest.raises(ValueError, match="outside"):
        residual.member_table(5, [[5]])
    many = residual.member_tables(5, sets + [[0], [2]])
    assert len(many) == 2 and many[0].tolist() == t.tolist() and many[1].tolist() == [1, 0, 2, 0, 0]
    assert all(int(x.max()) < 0x80 for x in many)
    assert len(residual.member_tables(5, [])) == 1


def test_explained_frame_columns_arithmetic_and_empty_sample():
    assert residual.EXPLAINED_COLUMNS == [
        "min_coverage", "num_present_organisms", "num_hashes", "num_hashes_in_database", "num_hashes_explained",
        "num_hashes_unexplained", "abund_total", "abund_in_database", "abund_explained", "abund_unexplained",
        "f_hashes_in_database", "f_hashes_explained", "f_abund_in_database", "f_abund_explained"]
    totals = np.zeros((8, 2), dtype=np.uint64)
    totals[7] = (60, 300)
    totals[0] = (10, 80)   # coverage 0.1 comes first in the call below: bit 0
    totals[1] = (40, 250)  # coverage 1.0: bit 1
    df = residual.explained_frame([0.1, 1.0], [3, 2], totals, n_hashes=100, abund_total=400)
    assert list(df.columns) == residual.EXPLAINED_COLUMNS
    assert df["min_coverage"].tolist() == [1.0, 0.1]  # coverage descending
    assert df.iloc[0].tolist() == [1.0, 2, 100, 60, 40, 60, 400, 300, 250, 150, 0.6, 0.4, 0.75, 0.625]
    assert df.iloc[1].tolist() == [0.1, 3, 100, 60, 10, 90, 400, 300, 80, 320, 0.6, 0.1, 0.75, 0.2]
    # one totals array per coverage (more than seven coverages): call set c is bit c % 7 of totals[c]
    second = np.zeros((8, 2), dtype=np.uint64)
    second[7] = (60, 300)
    second[0] = (5, 7)
    covs = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3]
    df = residual.explained_frame(covs, [1] * 8, [totals] * 7 + [second], 100, 400)
    assert df["num_hashes_explained"].tolist() == [10, 40, 0, 0, 0, 0, 0, 5] and df["abund_explained"].tolist()[-1] == 7
    empty = residual.explained_frame([1.0], [0], np.zeros((8, 2), dtype=np.uint64), 0, 0)
    assert empty.iloc[0].tolist() == [1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0]


HASHES = np.array([3, 8, 21, 34, 55, 89, 144, 233], dtype=np.uint64)
ABUND = np.array([5, 1, 9, 2, 7, 3, 4, 6], dtype=np.int64)
FLAGS = np.array([0x81, 0, 0x80, 0x83, 0x82, 0, 0x81, 0x80], dtype=np.uint8)


def test_residual_signature_of_a_hand_made_sample(tmp_path):
    sig = sigio.make_signature(HASHES, ksize=31, scaled=1000, name="hand made", abundances=ABUND)
    res = residual.residual_signature(sig, FLAGS, 0, 0.5)  # bit 0 clear: hashes 1, 2, 4, 5, 7
    assert res.name == "hand made residual"
    assert res.minhash.mins.tolist() == [8, 21, 55, 89, 233] and res.minhash.abundances.tolist() == [1, 9, 7, 3, 6]
    assert (res.minhash.ksize, res.minhash.scaled, res.minhash.seed) == (31, 1000, sig.minhash.seed)
    assert res.minhash.max_hash == sig.minhash.max_hash
    res1 = residual.residual_signature(sig, FLAGS, 1, 1.0)
    assert res1.minhash.mins.tolist() == [3, 8, 21, 89, 144, 233] and res1.minhash.abundances.tolist() == [5, 1, 9, 3, 4, 6]
    with pytest.raises(ValueError, match="flags"):
        residual.residual_signature(sig, FLAGS[:7], 0, 0.5)
    # a sample without abundances gives a signature without them
    bare = residual.residual_signature(sigio.make_signature(HASHES, ksize=31, scaled=1000, name="bare"), FLAGS, 0, 0.5)
    assert bare.minhash.abundances is None and bare.minhash.mins.tolist() == [8, 21, 55, 89, 233] and bare.name == "bare residual"


@pytest.mark.parametrize("with_abundance", [True, False])
def test_residual_zip_round_trips_as_a_sample(tmp_path, with_abundance):
    sig = sigio.make_signature(HASHES, ksize=31, scaled=1000, name="s", abundances=ABUND if with_abundance else None)
    totals = np.zeros((8, 2), dtype=np.uint64)
    totals[7] = (6, 33)
    totals[0] = (3, 11)
    totals[1] = (2, 9)
    frame = residual.write_outputs(str(tmp_path), sig, [1.0, 0.5], [np.array([0]), np.array([0, 1])], [FLAGS, FLAGS], [totals, totals], 0.5)
    assert sorted(os.listdir(tmp_path)) == [residual.RESIDUAL_NAME, residual.EXPLAINED_NAME] == ["residual.sig.zip", "sample_explained.tsv"]
    path = str(tmp_path / residual.RESIDUAL_NAME)
    assert sigio.zip_has_manifest(path)
    back = utils.load_signature_with_ksize(path, 31)
    assert back.name == "s residual" and back.minhash.scaled == 1000
    assert np.asarray(back.minhash.mins).tolist() == [3, 8, 21, 89, 144, 233]  # coverage 0.5 is call set 1: bit 1 clear
    if with_abundance:
        assert np.asarray(back.minhash.abundances).tolist() == [5, 1, 9, 3, 4, 6]
        assert frame["abund_total"].tolist() == [37, 37]
    else:
        assert back.minhash.abundances is None and back.minhash.mean_abundance is None
        assert frame["abund_total"].tolist() == [8, 8]  # no abundances: every hash counts once
    assert frame["num_present_organisms"].tolist() == [1, 2] and frame["num_hashes_explained"].tolist() == [3, 2]
    import pandas as pd

    assert list(pd.read_csv(tmp_path / residual.EXPLAINED_NAME, sep="\t").columns) == residual.EXPLAINED_COLUMNS


def test_call_sets_map_table_rows_to_manifest_rows():
    import pandas as pd

    names = ["a", "b", "c", "b", "d"]  # a duplicate organism name: both rows named b are in a table that lists b
    table = pd.DataFrame({"organism_name": ["b", "b", "d"], "in_sample_est": [False, True, True]})
    none = pd.DataFrame({"organism_name": ["b", "b", "d"], "in_sample_est": [False, False, False]})
    got = residual.call_sets_of(names, [table, none])
    assert got[0].tolist() == [3, 4] and got[1].tolist() == []
