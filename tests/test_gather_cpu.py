"""`yacht run --gather` without a GPU: the two oracles of tests/gather_oracle.py against each other and against the
consequences of the contract (explain_oracle for the sums), the library's new symbols and their argument handling, the
command line and its refusals before any device work, the host-side argument checks of RefDB.gather, and the pure numpy /
pandas side (yacht_amd/gather.py): the candidate table and the profile's frame."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
from explain_oracle import explain_oracle
from gather_oracle import NOBODY, ROW_DTYPE, gather_oracle, gather_sets

from yacht_amd import _lib, engine, gather, run_YACHT

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")


def small_database(rng):
    """3..12 references drawn from a pool of 40 hashes (heavy sharing), a sample of most of the pool plus hashes no
    reference holds, a random candidate set (sometimes empty, sometimes all) and abundances."""
    n = int(rng.integers(3, 13))
    pool = np.arange(10, 50, dtype=np.uint64)
    refs = [np.sort(rng.choice(pool, size=int(rng.integers(0, 16)), replace=False)) for _ in range(n)]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in refs])
    values = np.concatenate(refs) if int(offsets[-1]) else np.zeros(0, np.uint64)
    sample = np.sort(np.concatenate([rng.choice(pool, size=int(rng.integers(0, 36)), replace=False), np.arange(100, 105, dtype=np.uint64)]))
    cand = (rng.random(n) < rng.choice([0.0, 0.3, 0.7, 1.0])).astype(np.uint8)
    abund = rng.integers(0, 1000, sample.size)
    return values, offsets, sample, cand, abund


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_the_two_oracles_agree_and_the_contract_has_its_consequences():
    rng = np.random.default_rng(701)
    seen_rows = seen_ties = seen_more = 0
    for case in range(200):
        values, offsets, sample, cand, abund = small_database(rng)
        for ab in (abund, None):
            stats = {}
            full = gather_oracle(values, offsets, sample, cand, ab, stats=stats)
            assert same(full, gather_sets(values, offsets, sample, cand, ab)), case
            rows, more, owner = full
            assert rows.dtype == ROW_DTYPE and not more
            seen_rows += len(rows)
            seen_ties += stats["n_tie_rounds"]
            # n_unique never increases; row 0's is the largest overlap among the candidates
            assert (np.diff(rows["n_unique"].astype(np.int64)) <= 0).all(), case
            overlaps = [np.isin(sample, values[int(offsets[j]):int(offsets[j + 1])]).sum() for j in range(cand.size) if cand[j]]
            assert (int(rows["n_unique"][0]) if len(rows) else 0) == (max(overlaps) if overlaps else 0), case
            assert (rows["n_unique"] <= rows["n_overlap"]).all() and len(set(rows["ref"].tolist())) == len(rows)
            # the sums and the owners against explain's totals and flags for the member table cand != 0 in bit 3
            flags, totals = explain_oracle(values, offsets, sample, (cand != 0).astype(np.uint8) << 3, ab)
            assert int(rows["n_unique"].sum()) == int(totals[3, 0]) and int(rows["w_unique"].sum()) == int(totals[3, 1]), case
            assert np.array_equal(owner != NOBODY, (flags & 8) != 0), case
            for k, r in enumerate(rows):  # a row's numbers are those of the hashes it owns
                mine = owner == r["ref"]
                assert int(mine.sum()) == int(r["n_unique"])
                assert int((abund[mine] if ab is not None else np.ones(int(mine.sum()), dtype=np.int64)).sum()) == int(r["w_unique"])
            # the stops
            for min_hits, cap in ((2, None), (1, 1), (1, len(rows)), (3, 2), (1, 0)):
                got = gather_oracle(values, offsets, sample, cand, ab, min_hits=min_hits, cap_rows=cap)
                assert same(got, gather_sets(values, offsets, sample, cand, ab, min_hits=min_hits, cap_rows=cap)), (case, min_hits, cap)
                keep = int((rows["n_unique"] >= min_hits).sum())
                k = keep if cap is None else min(keep, cap)
                assert np.array_equal(got[0], rows[:k]) and got[1] == (cap is not None and keep > cap), (case, min_hits, cap)
                assert np.array_equal(got[2], np.where(np.isin(owner, rows["ref"][:k]), owner, NOBODY)), (case, min_hits, cap)
                seen_more += got[1]
    assert seen_rows > 500 and seen_ties > 50 and seen_more > 100  # (the cases are not degenerate)


def test_library_exposes_the_entries_and_rejects_bad_arguments():
    lib = _lib.load()
    assert hasattr(lib, "yh_gather") and hasattr(lib, "yh_gather_device")
    assert lib.yh_abi_version() == 8
    buf = np.zeros(16, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    n_rows, more = C.c_uint64(7), C.c_int(7)
    assert lib.yh_gather(None, p, None, 0, p, 1, p, 4, None, C.byref(n_rows), C.byref(more)) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_gather_device(None, p, None, 0, p, 1, p, 4, None, C.byref(n_rows), C.byref(more)) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()


def test_header_declares_what_the_binding_types():
    with open(HEADER) as f:
        text = f.read()
    assert "int yh_gather_device(" in text and "int yh_gather(" in text and "#define YH_ABI_VERSION 8" in text
    assert "typedef struct yh_gather_row" in text and "#define YH_GATHER_ROUNDS_PER_SYNC 32" in text
    assert "yh_gather / yh_gather_device" in text  # its row of the interleaving table
    assert len(_lib.SIGNATURES["yh_gather"][1]) == 11 and len(_lib.SIGNATURES["yh_gather_device"][1]) == 11
    assert _lib.YH_GATHER_ROUNDS_PER_SYNC == 32 and _lib.YH_GATHER_NOBODY == NOBODY
    assert engine.GATHER_ROW_DTYPE == ROW_DTYPE and engine.GATHER_ROW_DTYPE.itemsize == 24


def _parse(*argv):
    p = argparse.ArgumentParser()
    run_YACHT.add_arguments(p)
    return p.parse_args(["--json", "x.json", "--sample_file", "a.sig.zip", *argv])


def test_parser_takes_the_options_with_their_defaults():
    args = _parse()
    assert args.gather is False and args.gather_min_hits == 1 and args.gather_coverage is None
    assert gather.gather_options(args) is None
    args = _parse("--gather", "--gather_min_hits", "5", "--gather_coverage", "0.1", "1", "--min_coverage_list", "1", "0.5", "0.1")
    assert gather.gather_options(args) == ([1.0, 0.1], 5)
    assert gather.gather_options(_parse("--gather", "--min_coverage_list", "0.5", "1", "0.5")) == ([1.0, 0.5], 1)
    assert gather.gather_options(_parse("--gather", "--residual", "--abundance")) == ([1.0, 0.5, 0.1, 0.05, 0.01], 1)


def test_option_validation_comes_before_any_work(tmp_path):
    with pytest.raises(ValueError, match="not one of the --min_coverage_list"):
        gather.gather_options(_parse("--gather", "--gather_coverage", "0.2"))
    with pytest.raises(ValueError, match="needs --gather"):
        gather.gather_options(_parse("--gather_coverage", "0.1"))
    with pytest.raises(ValueError, match="at least 1"):
        gather.gather_options(_parse("--gather", "--gather_min_hits", "0"))
    # through the command's main: nothing is read (the config does not exist) and nothing is written
    for argv in (["--gather", "--gather_coverage", "0.2"], ["--gather_coverage", "0.1"], ["--gather", "--gather_min_hits", "0"]):
        args = _parse(*argv, "--outdir", str(tmp_path / "out"))
        with pytest.raises(ValueError):
            run_YACHT.main(args)
        assert not (tmp_path / "out").exists()


def test_a_cohort_is_refused_before_anything_is_written(tmp_path):
    p = argparse.ArgumentParser()
    run_YACHT.add_arguments(p)
    args = p.parse_args(["--json", "x.json", "--sample_file", "a.sig.zip", "b.sig.zip", "--gather", "--outdir", str(tmp_path / "out")])
    with pytest.raises(ValueError, match="one sample file, not 2"):
        run_YACHT.main(args)
    assert not (tmp_path / "out").exists()
    args.gather = False  # (the refusal is the flag's: without it the same arguments give no plan and no error here)
    assert gather.gather_options(args, 2) is None


def test_binding_checks_its_arguments_on_the_host():
    assert engine.check_candidates([0, 2, 1, 0], 4).tolist() == [0, 1, 1, 0]
    assert engine.check_candidates(np.array([True, False]), 2).dtype == np.uint8
    with pytest.raises(ValueError, match="one entry per reference"):
        engine.check_candidates([1, 0], 3)
    with pytest.raises(ValueError, match="booleans or integers"):
        engine.check_candidates(np.array([0.5, 1.0]), 2)
    assert engine.check_gather_limits(1, None, 9) == (1, 9) and engine.check_gather_limits(3, 4, 9) == (3, 4)
    assert engine.check_gather_limits(1, 100, 9) == (1, 9) and engine.check_gather_limits(1, 0, 9) == (1, 0)
    for bad in (0, -1, 2 ** 32, 1.5):
        with pytest.raises(ValueError, match="min_hits"):
            engine.check_gather_limits(bad, None, 9)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="cap_rows"):
            engine.check_gather_limits(1, bad, 9)


def test_candidate_table():
    assert gather.candidate_table(5, [3, 0]).tolist() == [1, 0, 0, 1, 0]
    assert gather.candidate_table(3, []).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="outside"):
        gather.candidate_table(3, [3])


def _rows(*rows):
    out = np.zeros(len(rows), dtype=engine.GATHER_ROW_DTYPE)
    for k, (ref, n_ov, n_un, w) in enumerate(rows):
        out[k] = (ref, n_ov, n_un, 0, w)
    return out


def test_frame_from_hand_made_rows():
    names = ["org_a", "org_b", "org_c", "org_d"]
    covs = [0.1, 1.0]  # (given ascending: the frame sorts them descending)
    rows = [_rows((2, 50, 50, 400), (0, 40, 10, 25), (3, 8, 1, 2 ** 40)), _rows((2, 50, 50, 400))]
    frame = gather.gather_frame(covs, rows, names, 200, 1000)
    assert list(frame.columns) == gather.GATHER_COLUMNS
    assert frame["min_coverage"].tolist() == [1.0, 0.1, 0.1, 0.1] and frame["rank"].tolist() == [0, 0, 1, 2]
    assert frame["organism_name"].tolist() == ["org_c", "org_c", "org_a", "org_d"]
    assert frame["num_overlap"].tolist() == [50, 50, 40, 8] and frame["num_unique"].tolist() == [50, 50, 10, 1]
    assert frame["f_overlap_of_sample"].tolist() == [50 / 200, 50 / 200, 40 / 200, 8 / 200]
    assert frame["f_unique_of_sample"].tolist() == [50 / 200, 50 / 200, 10 / 200, 1 / 200]
    assert frame["abund_sum_unique"].tolist() == [400, 400, 25, 2 ** 40]
    assert frame["mean_abund_unique"].tolist() == [8.0, 8.0, 2.5, float(2 ** 40)]
    assert frame["f_unique_weighted"].tolist() == [0.4, 0.4, 0.025, 2 ** 40 / 1000]
    # an empty sample: the fractions are 0; no rows at all: the columns alone
    empty = gather.gather_frame([1.0], [_rows((1, 0, 0, 0))], names, 0, 0)
    assert empty[["f_overlap_of_sample", "f_unique_of_sample", "mean_abund_unique", "f_unique_weighted"]].values.tolist() == [[0.0] * 4]
    none = gather.gather_frame([1.0, 0.5], [_rows(), _rows()], names, 10, 10)
    assert list(none.columns) == gather.GATHER_COLUMNS and len(none) == 0
