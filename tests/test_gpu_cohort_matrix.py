"""`yacht run --matrix` over a cohort, on the GPU.

At the level of cohort._Device: 300 synthetic samples (two blocks) against 1 500 references; the tables matrix.Collector makes
from the blocks' device-resident cells equal the pivot of the host's own per-sample tables (hyp_test_native on the blocks' rows,
abundance.abundance_columns on their depths), over three user coverages behind a forced 1.0, with and without abundances, and
with a row capacity of 1 that sends the first block through the dense fallback.

From files, on the fixture cohort of tests/test_gpu_cohort.py with --abundance --matrix: the wide tables equal the pivot of the
same run's cohort_presence.tsv, cohort_prevalence.tsv its group-by; --matrix_min_samples 2 drops exactly the organisms of
prevalence 1; the default route and YACHT_COHORT_MATRIX=host, each in a fresh child process, leave the same results/ tree; a run
without the flag leaves that tree minus the four tables; and a database with a repeated organism name leaves the same files by
both routes."""
import json
import os
import shutil
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pandas as pd
import pytest
from test_gpu_cohort import trained as fixture_cohort  # noqa: F401  (the module's fixture, made again for this module)
from test_gpu_cohort_residual_device import _same_tree, _synthetic

from yacht_amd import abundance, cli, cohort, matrix
from yacht_amd.engine import MATRIX_CELL_DTYPE, RefDB
from yacht_amd.hypothesis_recovery_src import hyp_test_native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVS = [1.0, 0.5, 0.1, 0.02]  # (1.0 stands for the forced coverage in front: the last three are the user's)
N_USER = 3
BIT, MIN_SAMPLES = 1, 2
MATRIX_FILES = [matrix.PREVALENCE_NAME, matrix.PRESENCE_NAME, matrix.NUM_MATCHES_NAME, matrix.ABUNDANCE_NAME]


# ---- cohort._Device ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic(hip_lib):
    values, offsets, samples, abunds = _synthetic(300)
    abunds = [np.ones(s.size, np.uint32) if a is None else a for s, a in zip(samples, abunds)]
    with RefDB(values, offsets) as db:
        n_max = int(np.max(db.sizes))
        tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        yield db, samples, abunds, tab


def _blocks(db, tab, samples, abunds, want_abundance, cap=0):
    dev = cohort._Device(db, COVS, 31, 0.95, tab[5], cap=cap, abund_samples=256 if want_abundance else 0, matrix_sets=N_USER)
    timer = defaultdict(float)
    gots = []
    for lo in (0, 256):
        ab = abunds[lo:lo + 256] if want_abundance else None
        gots.append((lo, dev.collect(dev.launch(samples[lo:lo + 256], ab, None, sample_base=lo), timer)))
    return dev, gots, timer


def _host_pivot(gots, n_refs, n_samples, want_abundance):
    """[coverage][reference][sample] presence, num_matches and relative abundance from the blocks' rows, by the host's own code."""
    pres = np.zeros((N_USER, n_refs, n_samples), dtype=np.uint8)
    nm = np.zeros((N_USER, n_refs, n_samples), dtype=np.uint32)
    rel = np.zeros((N_USER, n_refs, n_samples), dtype=np.float64)
    for lo, got in gots:
        rows = got[0]
        smp, ref = rows[:, 0].astype(np.int64) + lo, rows[:, 1].astype(np.int64)
        for c, cov in enumerate(COVS[-N_USER:]):
            present = np.asarray(hyp_test_native(rows[:, 3].astype(np.int64), rows[:, 4].astype(np.int64), 31, 0.99, 0.95, cov)[0], dtype=bool)
            assert np.array_equal(present, got[2][len(COVS) - N_USER + c].astype(bool))
            pres[c, ref[present], smp[present]] = 1
            nm[c, ref[present], smp[present]] = rows[present, 4]
            if want_abundance:
                for s in np.unique(smp):
                    sel = smp == s
                    cols = abundance.abundance_columns(got[4][0][sel], got[4][1][sel], got[4][2][sel], rows[sel, 2], rows[sel, 4], present[sel], 1)
                    rel[c, ref[sel], s] = cols["relative_abundance"].to_numpy()
    return pres, nm, rel


def _tables(dev, db, n_samples, want_abundance, timer, min_samples=MIN_SAMPLES):
    col = matrix.Collector(db.n_refs, n_samples, N_USER, want_abundance, False)
    for cells in dev.matrix_cells:
        col.add_device(cells)
    return col.tables(BIT, min_samples, db, dev.torch, dev.dev, timer)


def _check_tables(tables, pivot, n_samples, want_abundance):
    prev, kept, presence, n_match, rel, stats = tables
    pres, nm, want_rel = pivot
    assert np.array_equal(prev, pres.sum(axis=2, dtype=np.uint32))
    assert np.array_equal(kept, prev[BIT] >= MIN_SAMPLES)
    # the cohort exercises the cut: some organisms kept, one in two or more samples, one in fewer than all, one dropped
    assert kept.sum() >= 2 and (prev[BIT] >= 2).any() and (prev[BIT][kept] < n_samples).any() and (prev[BIT] == 1).any()
    assert np.array_equal(presence, pres[BIT][kept]) and np.array_equal(n_match, nm[BIT][kept])
    if not want_abundance:
        assert rel is None and stats is None
        return
    assert np.array_equal(rel.view(np.uint64), want_rel[BIT][kept].view(np.uint64))
    for c in range(N_USER):
        sums = want_rel[c].sum(axis=0)
        assert (np.isclose(sums, 1.0, rtol=0, atol=1e-12) | (sums == 0)).all()
        on = prev[c] > 0
        mean, mx = matrix.reduce_rel(want_rel[c][on], n_samples)
        assert np.array_equal(stats[c][0].view(np.uint64), mean.view(np.uint64)) and np.array_equal(stats[c][1], mx)


@pytest.mark.parametrize("want_abundance", [False, True], ids=["plain", "abundance"])
def test_device_tables_equal_the_host_pivot(synthetic, want_abundance):
    db, samples, abunds, tab = synthetic
    dev, gots, timer = _blocks(db, tab, samples, abunds, want_abundance)
    assert timer["dense_fallback_blocks"] == 0 and len(dev.matrix_cells) == 2 and timer["gpu_matrix"] > 0
    pivot = _host_pivot(gots, db.n_refs, len(samples), want_abundance)
    tables = _tables(dev, db, len(samples), want_abundance, timer)
    _check_tables(tables, pivot, len(samples), want_abundance)
    # the same cells through the numpy route: the same tables
    cells = dev.torch.cat(dev.matrix_cells).cpu().numpy().reshape(-1).view(MATRIX_CELL_DTYPE)
    assert cells.size == int(pivot[0].any(axis=0).sum()) and (cells["sample"] >= 256).any()
    for a, b in zip(tables[:5], matrix.tables_numpy(cells, db.n_refs, len(samples), N_USER, BIT, MIN_SAMPLES, want_abundance)[:5]):
        assert (a is None and b is None) or (a.dtype == b.dtype and a.tobytes() == b.tobytes())


def test_a_row_capacity_of_one_makes_the_cells_again(synthetic):
    db, samples, abunds, tab = synthetic
    dev, gots, timer = _blocks(db, tab, samples, abunds, True, cap=1)
    assert timer["dense_fallback_blocks"] >= 1 and len(dev.matrix_cells) == 2
    _check_tables(_tables(dev, db, len(samples), True, timer), _host_pivot(gots, db.n_refs, len(samples), True), len(samples), True)


# ---- from files --------------------------------------------------------------------------------------------------------------
OPTS = ["--abundance", "--matrix", "--min_coverage_list", "1", "0.05", "0.001"]
USER = [1.0, 0.05, 0.001]


def _run(cfg, files, outdir, *opts):
    outdir.mkdir()
    assert cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(outdir), *opts]) == 0
    return outdir / "results"


def _read(path):
    return pd.read_csv(path, sep="\t", float_precision="round_trip")


def _check_files(res, cfg, files, coverage, min_samples=1):
    stems = [cohort.sample_stem(str(f)) for f in files]
    names = pd.read_csv(json.load(open(cfg))["manifest_file_path"], sep="\t")["organism_name"].tolist()
    long = _read(res / "cohort_presence.tsv")
    # cohort_prevalence.tsv = the group-by of the long table, coverage descending, then database order
    table = _read(res / matrix.PREVALENCE_NAME)
    assert list(table.columns) == matrix.PREVALENCE_COLUMNS + matrix.PREVALENCE_ABUNDANCE_COLUMNS
    want_rows = []
    for cov in USER:
        part = long[long["min_coverage"] == cov]
        for name in names:
            hit = part[part["organism_name"] == name]
            if len(hit):
                rel = np.zeros(len(stems))
                rel[[stems.index(s) for s in hit["sample"]]] = hit["relative_abundance"].to_numpy()
                want_rows.append((cov, name, len(hit), len(hit) / len(stems), rel.sum() / len(stems), rel.max()))
    assert len(want_rows) == len(table) and len(table) > 0
    for got, want in zip(table.itertuples(index=False), want_rows):
        assert tuple(got)[:4] == want[:4], want
        assert abs(got[4] - want[4]) <= 1e-15 and got[5] == want[5], want
    # the wide tables = the pivot of the long table at the coverage, rows in database order
    part = long[long["min_coverage"] == coverage]
    counts = part.groupby("organism_name").size()
    kept = [n for n in names if counts.get(n, 0) >= min_samples]  # (may be empty: a header and no row)
    for file_name, column in ((matrix.PRESENCE_NAME, None), (matrix.NUM_MATCHES_NAME, "num_matches"), (matrix.ABUNDANCE_NAME, "relative_abundance")):
        wide = _read(res / file_name)
        assert list(wide.columns) == ["organism_name"] + stems and wide["organism_name"].tolist() == kept, file_name
        want = np.zeros((len(kept), len(stems)))
        for row in part.itertuples(index=False):
            if row.organism_name in kept:
                want[kept.index(row.organism_name), stems.index(row.sample)] = 1 if column is None else getattr(row, column)
        got = wide[stems].to_numpy(dtype=np.float64)
        assert np.array_equal(got, want), file_name
        assert not got[:, stems.index("none")].any()
        if column == "relative_abundance" and min_samples == 1:
            sums = got.sum(axis=0)
            assert (np.isclose(sums, 1.0, rtol=0, atol=1e-12) | (sums == 0)).all() and ((sums != 0).any() or not kept)
    return counts


def test_fixture_cohort_tables_equal_the_long_table(hip_lib, fixture_cohort, tmp_path):  # noqa: F811
    tmp, cfg, files = fixture_cohort
    res = _run(cfg, files, tmp_path / "default", *OPTS)
    counts = _check_files(res, cfg, files, 0.001)
    assert len(counts) >= 1  # (the smallest coverage calls some organism present)
    mid =_run(cfg, files, tmp_path / "middle", *OPTS, "--matrix_coverage", "0.05")
    _check_files(mid, cfg, files, 0.05)
    assert (mid / matrix.PREVALENCE_NAME).read_bytes() == (res / matrix.PREVALENCE_NAME).read_bytes()
    two = _run(cfg, files, tmp_path / "two", *OPTS, "--matrix_min_samples", "2")
    _check_files(two, cfg, files, 0.001, min_samples=2)
    assert (two / matrix.PREVALENCE_NAME).read_bytes() == (res / matrix.PREVALENCE_NAME).read_bytes()  # the cut is not its business
    dropped = set(_read(res / matrix.PRESENCE_NAME)["organism_name"]) - set(_read(two / matrix.PRESENCE_NAME)["organism_name"])
    assert dropped == {n for n, k in counts.items() if k == 1}
    # without the flag: the same tree minus the four tables
    plain = _run(cfg, files, tmp_path / "plain", *[o for o in OPTS if o != "--matrix"])
    assert not any((plain / n).exists() for n in MATRIX_FILES)
    shutil.copytree(res, tmp_path / "minus")
    for n in MATRIX_FILES:
        os.remove(tmp_path / "minus" / n)
    _same_tree(str(plain), str(tmp_path / "minus"), "without the flag")


def test_the_default_and_the_host_route_leave_the_same_tree(hip_lib, fixture_cohort, tmp_path):  # noqa: F811
    """Each in a fresh child process, side by side."""
    tmp, cfg, files = fixture_cohort
    running = []
    for name, mode in (("device", None), ("host", "host")):
        outdir = tmp_path / name
        outdir.mkdir()
        env = {k: v for k, v in os.environ.items() if k != matrix.ENV}
        if mode is not None:
            env[matrix.ENV] = mode
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        running.append(subprocess.Popen([sys.executable, "-m", "yacht_amd", "run", "--json", str(cfg), "--sample_file", *map(str, files),
                                         "--num_threads", "2", "--outdir", str(outdir), *OPTS, "--matrix_min_samples", "2"], env=env, cwd=ROOT,
                                        stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    for child in running:
        _out, err = child.communicate()
        assert child.returncode == 0, err[-2000:]
    names = _same_tree(str(tmp_path / "device" / "results"), str(tmp_path / "host" / "results"), "device against host")
    assert all(n in names for n in MATRIX_FILES)


def test_a_repeated_organism_name_leaves_the_same_files_by_both_routes(hip_lib, fixture_cohort, tmp_path, monkeypatch):  # noqa: F811
    """Two references under one name (as tests/test_gpu_cohort.py builds them): the host recomputes such a sample's tables, the
    device skips its cells and takes the host's; the wide tables keep one row per reference."""
    tmp, cfg, files = fixture_cohort
    conf = json.load(open(cfg))
    man = pd.read_csv(conf["manifest_file_path"], sep="\t")
    probe = _run(cfg, [files[1]], tmp_path / "probe", "--show_all")
    hit = set(pd.read_csv(probe / "result_all.txt", sep="\t")["organism_name"])
    have, miss = [n for n in man["organism_name"] if n in hit], [n for n in man["organism_name"] if n not in hit]
    assert have and miss
    man.loc[man["organism_name"] == miss[0], "organism_name"] = have[0]
    man.to_csv(tmp_path / "dup_manifest.tsv", sep="\t", index=False)
    conf["manifest_file_path"] = str(tmp_path / "dup_manifest.tsv")
    (tmp_path / "dup_config.json").write_text(json.dumps(conf))
    res = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv(matrix.ENV, "host")
        else:
            monkeypatch.delenv(matrix.ENV, raising=False)
        res[mode] = _run(tmp_path / "dup_config.json", files, tmp_path / mode, *OPTS)
    monkeypatch.delenv(matrix.ENV, raising=False)
    names = _same_tree(str(res["device"]), str(res["host"]), "repeated name")
    assert all(n in names for n in MATRIX_FILES)
    wide = _read(res["device"] / matrix.PRESENCE_NAME)
    assert len(wide) >= 1
    order = iter(man["organism_name"].tolist())
    assert all(any(name == n for n in order) for name in wide["organism_name"])  # database order: a subsequence of the manifest's names
