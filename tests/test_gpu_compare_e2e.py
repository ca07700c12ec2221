"""`yacht compare` and `yacht run --compare` from files to files, on the GPU.

Six small samples written with sigio, two of them without abundances: the files `yacht compare` writes equal those the
writers make from the numpy oracle's integers (tests/compare_cases.py), and a few values are worked out from Python sets.
The cohort run on the 20-genome fixture database (tests/test_gpu_cohort.py's) with --compare --residual: its
cohort_compare.tsv is `yacht compare`'s byte for byte, its cohort_compare_residual.tsv equals `yacht compare` over the
residual.sig.zip files the same run wrote (a sample without overlap has none: it keeps all its hashes), and panels of two
samples leave the same bytes."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest
from compare_cases import oracle
from test_gpu_cohort import trained  # noqa: F401  (the module's fixture, made again for this module)

from yacht_amd import cli, cohort, compare, residual, sigio

pytestmark = pytest.mark.gpu

FILES = [compare.TABLE_NAME] + [compare.MATRIX_NAME.format(m) for m in compare.MATRIX_METRICS]


def _read(path):
    return pd.read_csv(path, sep="\t", float_precision="round_trip")


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def six(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("compare_six")
    rng = np.random.default_rng(77)
    top = sigio.max_hash_for_scaled(1000)
    pool = np.unique(rng.integers(0, top, 4000, dtype=np.uint64))
    samples, abunds, paths = [], [], []
    for s, n in enumerate((900, 1500, 40, 2500, 700, 1200)):
        mins = np.sort(rng.choice(pool, size=n, replace=False))
        ab = None if s in (1, 4) else 1 + rng.integers(0, 30, n)
        p = tmp / f"smp{s}.sig.zip"
        sigio.write_sig_zip([sigio.make_signature(mins, ksize=31, scaled=1000, name=f"sample {s}", abundances=ab)], str(p))
        samples.append(mins), abunds.append(ab), paths.append(p)
    return tmp, samples, abunds, paths


def test_yacht_compare_writes_the_oracles_files(hip_lib, six, tmp_path):
    tmp, samples, abunds, paths = six
    out = tmp_path / "out"
    out.mkdir()
    assert cli.main(["compare", "--sample_file", *map(str, paths), "--ksize", "31", "--outdir", str(out), "--num_threads", "2"]) == 0
    res = out / "results"
    assert sorted(os.listdir(res)) == sorted(FILES)
    cells, s_a, _ = oracle(dict(a=samples, b=None, a_ab=abunds, b_ab=None, a_keep=None, b_keep=None, keep_and=0, keep_eq=0))
    mask = (1 << 64) - 1
    want_cells = np.array([[(n, mn, d & mask, d >> 64) for n, mn, d in row] for row in cells], dtype=compare.CELL_DTYPE)
    want_self = np.array([(n, sm, sq & mask, sq >> 64) for n, sm, sq in s_a], dtype=compare.SELF_DTYPE)
    want = tmp_path / "want"
    want.mkdir()
    stems = [f"smp{s}" for s in range(6)]
    compare.write_outputs(str(want), stems, want_cells, want_self, 31)
    for name in FILES:
        assert _bytes(res / name) == _bytes(want / name), name
    # a few values from Python sets and dicts
    table = _read(res / compare.TABLE_NAME)
    assert len(table) == 15 and table["sample_a"].tolist()[:5] == ["smp0"] * 5 and table["sample_b"].tolist()[:5] == stems[1:]
    row = table[(table["sample_a"] == "smp0") & (table["sample_b"] == "smp3")].iloc[0]
    a = dict(zip(map(int, samples[0]), map(int, abunds[0])))
    b = dict(zip(map(int, samples[3]), map(int, abunds[3])))
    both = set(a) & set(b)
    assert row["n_shared"] == len(both) > 100 and row["n_hashes_a"] == 900 and row["n_hashes_b"] == 2500
    assert row["jaccard"] == len(both) / len(set(a) | set(b)) and row["containment_a_in_b"] == len(both) / 900
    assert row["abund_sum_min"] == sum(min(a[h], b[h]) for h in both)
    assert row["bray_curtis"] == 1 - 2 * row["abund_sum_min"] / (sum(a.values()) + sum(b.values()))
    dot = sum(a[h] * b[h] for h in both)
    assert row["cosine"] == pytest.approx(dot / (sum(v * v for v in a.values()) ** 0.5 * sum(v * v for v in b.values()) ** 0.5), rel=1e-14)
    flat = table[(table["sample_a"] == "smp1") & (table["sample_b"] == "smp4")].iloc[0]  # neither tracks abundances
    assert flat["abund_sum_min"] == flat["n_shared"] and flat["bray_curtis"] == 1 - 2 * flat["n_shared"] / (1500 + 700)


COMPARE_FILES = FILES + [compare.RESIDUAL_TABLE_NAME]


def test_cohort_compare_with_residual_and_in_panels(hip_lib, trained, tmp_path, monkeypatch):  # noqa: F811
    tmp, cfg, files = trained
    stems = [cohort.sample_stem(str(p)) for p in files]
    opts = ["--compare", "--residual", "--min_coverage_list", "0.05", "0.001"]
    monkeypatch.delenv(compare.PANEL_BYTES_ENV, raising=False)
    runs = {}
    for mode in ("whole", "panels"):
        out = tmp_path / mode
        out.mkdir()
        if mode == "panels":
            monkeypatch.setenv(compare.PANEL_BYTES_ENV, "1")
            assert [len(p) for p in compare.plan_panels([100] * len(files), compare.panel_bytes())] == [2, 2, 1]
        assert cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(out), *opts]) == 0
        runs[mode] = out / "results"
    monkeypatch.delenv(compare.PANEL_BYTES_ENV, raising=False)
    for name in COMPARE_FILES:
        assert _bytes(runs["whole"] / name) == _bytes(runs["panels"] / name), name
    res = runs["whole"]
    # the same table as `yacht compare` over the same files
    plain = tmp_path / "plain"
    plain.mkdir()
    assert cli.main(["compare", "--sample_file", *map(str, files), "--ksize", "31", "--outdir", str(plain), "--num_threads", "2"]) == 0
    for name in FILES:
        assert _bytes(res / name) == _bytes(plain / "results" / name), name
    assert not (plain / "results" / compare.RESIDUAL_TABLE_NAME).exists()
    # the residual table: `yacht compare` over the residual.sig.zip files of this run
    left = tmp_path / "left"
    left.mkdir()
    left_files = []
    for stem, src in zip(stems, files):
        wrote = res / stem / residual.RESIDUAL_NAME
        assert wrote.exists() == (stem != "none")
        left_files.append(shutil.copyfile(wrote if wrote.exists() else src, left / f"{stem}.sig.zip"))
    assert cli.main(["compare", "--sample_file", *map(str, left_files), "--ksize", "31", "--outdir", str(left), "--num_threads", "2"]) == 0
    got, want = _read(res / compare.RESIDUAL_TABLE_NAME), _read(left / "results" / compare.TABLE_NAME)
    values = [c for c in compare.TABLE_COLUMNS if c not in ("sample_a", "sample_b")]
    assert got[values].equals(want[values]) and len(got) == 10
    full = _read(res / compare.TABLE_NAME)
    print("hashes per pair, all and left over:", full["n_hashes_a"].tolist(), got["n_hashes_a"].tolist())
    assert (got["n_hashes_a"] <= full["n_hashes_a"]).all() and (got["n_shared"] <= full["n_shared"]).all()
    assert got["sample_a"].tolist() == full["sample_a"].tolist() and got["sample_b"].tolist() == full["sample_b"].tolist()
