"""tests/matrix_cases.py on the CPU: its loop oracle against a brute-force pivot through pandas, every case inside the stated
shape limits, and yacht_amd/matrix.py's numpy route (what YACHT_COHORT_MATRIX=host builds the tables with) against the oracle.
No GPU."""
import ctypes as C
import os
import re

import matrix_cases as mc
import numpy as np
import pandas as pd
import pytest

from yacht_amd import _lib, matrix
from yacht_amd.engine import MATRIX_CELL_DTYPE

CELLS = mc.cells_cases()
PREV = mc.prevalence_cases()
FILL = mc.fill_cases()
ENTRIES = ("yh_matrix_cells_device", "yh_matrix_prevalence_device", "yh_matrix_fill_device")


def _ids(cases):
    return [c["name"] for c in cases]


def test_binding_and_header_agree():
    assert [len(_lib.SIGNATURES[name][1]) for name in ENTRIES] == [10, 8, 12]
    assert all(_lib.SIGNATURES[name][0] is C.c_int for name in ENTRIES)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        text = f.read()
    for name, want in (("YH_MATRIX_MAX_SETS", 32), ("YH_MATRIX_CHUNK", mc.CHUNK), ("YH_MATRIX_TILE", mc.TILE)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name) == want
    assert MATRIX_CELL_DTYPE == mc.CELL and MATRIX_CELL_DTYPE.itemsize == 24
    assert matrix.MAX_SETS == 32


def test_case_names_are_distinct_and_cover_the_edges():
    for cases in (CELLS, PREV, FILL):
        assert len(set(_ids(cases))) == len(cases)
    sizes = {len(c["rows"]) for c in CELLS} | {c["n_rows"] for c in CELLS}
    assert {0, 1, mc.CHUNK - 1, mc.CHUNK, mc.CHUNK + 1, 2 * mc.CHUNK + 1} <= sizes
    assert {len(c["present"]) for c in CELLS} >= {1, 7, 8, 32}
    assert any(c["n_rows"] > len(c["rows"]) for c in CELLS) and any(c["med"] is None for c in CELLS) and any(c["base"] == 256 for c in CELLS)
    assert {c["n_samples"] for c in PREV} >= {1, 63, 64, 65, 300}
    assert {int(c["kept"].sum()) for c in FILL} >= {0, 1, 5} and any(c["n_samples"] == 1 for c in FILL)


@pytest.mark.parametrize("case", CELLS + PREV + FILL, ids=_ids(CELLS) + [f"prev_{n}" for n in _ids(PREV)] + [f"fill_{n}" for n in _ids(FILL)])
def test_shape_limits(case):
    assert case["n_refs"] in (5, 300)
    if "rows" in case:
        cap = len(case["rows"])
        assert 1 <= cap <= mc.MAX_ROWS and case["present"].shape == (len(case["present"]), cap) and 1 <= len(case["present"]) <= 32
        assert case["med"] is None or (case["med"].shape == (cap,) and (case["med"] * 2 == np.floor(case["med"] * 2)).all() and case["med"].max() < 2 ** 33)
    else:
        cells = case["cells"]
        assert cells.dtype == mc.CELL and cells.size <= mc.MAX_ROWS and 1 <= case["n_samples"] <= mc.MAX_SAMPLES and 1 <= case["n_sets"] <= 32
        assert cells.size == 0 or int(cells["depth2"].max()) < 1 << 34
        ok = (cells["sample"] < case["n_samples"]) & (cells["ref"] < case["n_refs"])
        pairs = cells[ok][["sample", "ref"]].tolist()
        assert len(set(pairs)) == len(pairs)  # a (sample, reference) pair occurs at most once
        assert case["skip"] is None or case["skip"].shape == (case["n_samples"],)
        if "bit" in case:
            assert 0 <= case["bit"] < case["n_sets"] and case["kept"].shape == (case["n_refs"],)


# ---- the oracle against pandas ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CELLS, ids=_ids(CELLS))
def test_cells_oracle_against_pandas(case):
    rows, present = case["rows"], case["present"]
    n = min(case["n_rows"], len(rows))
    df = pd.DataFrame(rows[:n].astype(np.int64), columns=["sample", "ref", "overlap", "n_excl", "n_match"])
    df["mask"] = sum(((present[c, :n] != 0).astype(np.int64) << c) for c in range(len(present)))
    df["depth2"] = 0 if case["med"] is None else (2 * case["med"][:n]).astype(np.int64)
    df = df[(df["mask"] != 0) & (df["ref"] < case["n_refs"])]
    got = mc.cells_oracle(rows, case["n_rows"], present, case["med"], case["base"], case["n_refs"])
    assert got["sample"].tolist() == (df["sample"] + case["base"]).tolist() and got["ref"].tolist() == df["ref"].tolist()
    assert got["n_match"].tolist() == df["n_match"].tolist() and got["mask"].tolist() == df["mask"].tolist()
    assert got["depth2"].tolist() == df["depth2"].tolist()


def _long(cells, n_sets, n_samples, skip, n_refs):
    """One row per (cell, set bit) of the cells the passes take."""
    df = pd.DataFrame({k: cells[k].astype(np.int64) for k in cells.dtype.names})
    df = df[(df["sample"] < n_samples) & (df["ref"] < n_refs)]
    if skip is not None:
        df = df[np.asarray(skip)[df["sample"].to_numpy()] == 0]
    parts = [df[(df["mask"].to_numpy() >> c) & 1 == 1].assign(c=c) for c in range(n_sets)]
    return pd.concat(parts, ignore_index=True)


@pytest.mark.parametrize("case", PREV, ids=_ids(PREV))
def test_prevalence_oracle_against_pandas(case):
    prev, denom = mc.prevalence_oracle(case["cells"], case["n_sets"], case["n_samples"], case["skip"], case["n_refs"])
    long = _long(case["cells"], case["n_sets"], case["n_samples"], case["skip"], case["n_refs"])
    want_p = np.zeros_like(prev)
    for (c, ref), n in long.groupby(["c", "ref"]).size().items():
        want_p[c, ref] = n
    want_d = np.zeros_like(denom)
    for (c, smp), v in long.groupby(["c", "sample"])["depth2"].sum().items():
        want_d[c, smp] = v
    assert np.array_equal(prev, want_p) and np.array_equal(denom, want_d)


def _fill_inputs(case):
    _prev, denom = mc.prevalence_oracle(case["cells"], case["n_sets"], case["n_samples"], case["skip"], case["n_refs"])
    return mc.row_of_ref(case["kept"]), int(case["kept"].sum()), denom[case["bit"]]


@pytest.mark.parametrize("case", FILL, ids=_ids(FILL))
def test_fill_oracle_against_pandas(case):
    row_of, n_kept, den = _fill_inputs(case)
    presence, n_match, rel = mc.fill_oracle(case["cells"], case["bit"], case["n_samples"], case["skip"], row_of, n_kept, den, case["want_rel"])
    long = _long(case["cells"], case["n_sets"], case["n_samples"], case["skip"], case["n_refs"])
    long = long[(long["c"] == case["bit"]) & case["kept"][long["ref"].to_numpy()]]
    kept_refs = np.flatnonzero(case["kept"])

    def pivot(values):
        wide = long.assign(v=values).pivot_table(index="ref", columns="sample", values="v", aggfunc="sum", fill_value=0)
        return wide.reindex(index=kept_refs, columns=range(case["n_samples"]), fill_value=0).to_numpy()

    assert np.array_equal(presence, pivot(1)) and np.array_equal(n_match, pivot(long["n_match"].to_numpy()))
    if case["want_rel"]:
        d = den[long["sample"].to_numpy()].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = pivot(np.where(d != 0, long["depth2"].to_numpy().astype(np.float64) / d, 0.0))
        assert np.array_equal(rel.view(np.uint64), want.astype(np.float64).view(np.uint64))
        sums = rel.sum(axis=0)
        assert n_kept != case["n_refs"] or (np.isclose(sums, 1.0, rtol=0, atol=1e-12) | (sums == 0)).all()
    else:
        assert rel is None


# ---- matrix.py's numpy route against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CELLS, ids=_ids(CELLS))
def test_numpy_cells_equal_the_oracle(case):
    got = matrix.cells_from_rows(case["rows"], case["n_rows"], case["present"], case["med"], case["base"], case["n_refs"])
    want = mc.cells_oracle(case["rows"], case["n_rows"], case["present"], case["med"], case["base"], case["n_refs"])
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("case", PREV, ids=_ids(PREV))
def test_numpy_prevalence_equals_the_oracle(case):
    got = matrix.prevalence_numpy(case["cells"], case["n_sets"], case["n_samples"], case["skip"], case["n_refs"])
    want = mc.prevalence_oracle(case["cells"], case["n_sets"], case["n_samples"], case["skip"], case["n_refs"])
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("case", FILL, ids=_ids(FILL))
def test_numpy_fill_equals_the_oracle(case):
    row_of, n_kept, den = _fill_inputs(case)
    assert np.array_equal(matrix.row_of_ref_for(case["kept"]), row_of)
    got = matrix.fill_numpy(case["cells"], case["bit"], case["n_samples"], case["skip"], row_of, n_kept, den, case["want_rel"])
    want = mc.fill_oracle(case["cells"], case["bit"], case["n_samples"], case["skip"], row_of, n_kept, den, case["want_rel"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[2] is None) == (want[2] is None)
    if want[2] is not None:
        assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))


def test_numpy_tables_and_files(tmp_path):
    """tables_numpy on a small cohort of cells: the kept rows follow --matrix_min_samples, the statistics of every coverage do
    not depend on it, the files read back to the float64 values, and a repeated organism name keeps one row per reference."""
    case = next(c for c in FILL if c["name"] == "skipped_samples")
    cells, N, S, n_sets = case["cells"], case["n_refs"], case["n_samples"], case["n_sets"]
    one = matrix.tables_numpy(cells, N, S, n_sets, 2, 1, True)
    prev = one[0]
    m = int(np.median(prev[2][prev[2] > 0])) + 1  # (cuts about half of the organisms)
    two = matrix.tables_numpy(cells, N, S, n_sets, 2, m, True)
    assert np.array_equal(one[1], prev[2] >= 1) and np.array_equal(two[1], prev[2] >= m) and 0 < two[1].sum() < one[1].sum()
    assert np.array_equal(one[2][two[1][one[1]]], two[2]) and np.array_equal(one[4][two[1][one[1]]], two[4])
    for a, b in zip(one[5], two[5]):
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])
    sums = one[4].sum(axis=0)
    assert (np.isclose(sums, 1.0, rtol=0, atol=1e-12) | (sums == 0)).all() and (sums != 0).any()
    names = np.array([f"org {j // 2}" for j in range(N)], dtype=object)  # every name twice
    stems = [f"s{i}" for i in range(S)]
    covs = [1.0, 0.5, 0.25, 0.1, 0.05, 0.01]
    matrix.write_tables(str(tmp_path), names, stems, covs, *one)
    wide = pd.read_csv(tmp_path / matrix.ABUNDANCE_NAME, sep="\t", float_precision="round_trip")
    assert list(wide.columns) == ["organism_name"] + stems and wide["organism_name"].tolist() == names[one[1]].tolist()
    assert np.array_equal(wide[stems].to_numpy(dtype=np.float64).view(np.uint64), one[4].view(np.uint64))
    table = pd.read_csv(tmp_path / matrix.PREVALENCE_NAME, sep="\t", float_precision="round_trip")
    assert list(table.columns) == matrix.PREVALENCE_COLUMNS + matrix.PREVALENCE_ABUNDANCE_COLUMNS
    assert table["min_coverage"].tolist() == sorted(table["min_coverage"].tolist(), reverse=True)
    part = table[table["min_coverage"] == covs[2]]
    assert part["n_samples_present"].tolist() == prev[2][prev[2] > 0].tolist()
    assert np.array_equal(part["mean_relative_abundance"].to_numpy(), one[4].sum(axis=1) / S)
    assert (table["f_samples_present"] == table["n_samples_present"] / S).all()
    with pytest.raises(ValueError, match="--matrix_min_samples"):
        matrix.check_size(85205, 20000, True)
