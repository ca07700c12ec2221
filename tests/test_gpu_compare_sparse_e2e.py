"""`yacht compare` and `yacht run --compare --residual` write the same bytes on every route.

Six small samples written with sigio, two of them without abundances (the fixture idea of tests/test_gpu_compare_e2e.py,
made again here): cohort_compare.tsv and the four matrices under YACHT_COMPARE_ROUTE = dense, sparse and auto, whole and
with YACHT_COMPARE_PANEL_BYTES=1 (panels of two: many panel pairs, rectangular calls).  The cohort run on the 20-genome
fixture database with --compare --residual: cohort_compare_residual.tsv (keep bytes on both sides) under dense and sparse."""
import logging

import numpy as np
import pytest
from test_gpu_cohort import trained  # noqa: F401  (the module's fixture, made again for this module)

from yacht_amd import cli, compare, sigio

pytestmark = pytest.mark.gpu

FILES = [compare.TABLE_NAME] + [compare.MATRIX_NAME.format(m) for m in compare.MATRIX_METRICS]


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def six(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("compare_sparse_six")
    rng = np.random.default_rng(78)
    top = sigio.max_hash_for_scaled(1000)
    pool = np.unique(rng.integers(0, top, 4000, dtype=np.uint64))
    paths = []
    for s, n in enumerate((900, 1500, 40, 2500, 700, 1200)):
        mins = np.sort(rng.choice(pool, size=n, replace=False))
        ab = None if s in (1, 4) else 1 + rng.integers(0, 30, n)
        p = tmp / f"smp{s}.sig.zip"
        sigio.write_sig_zip([sigio.make_signature(mins, ksize=31, scaled=1000, name=f"sample {s}", abundances=ab)], str(p))
        paths.append(p)
    return paths


@pytest.mark.parametrize("panels", ["whole", "panels_of_two"])
def test_yacht_compare_writes_the_same_files_on_every_route(hip_lib, six, tmp_path, monkeypatch, caplog, panels):
    monkeypatch.delenv(compare.PANEL_BYTES_ENV, raising=False)
    if panels == "panels_of_two":
        monkeypatch.setenv(compare.PANEL_BYTES_ENV, "1")
    n_pairs = 1 if panels == "whole" else 6
    res = {}
    for route in ("dense", "sparse", "auto"):
        monkeypatch.setenv(compare.ROUTE_ENV, route)
        out = tmp_path / route
        out.mkdir()
        caplog.clear()
        with caplog.at_level(logging.INFO):
            assert cli.main(["compare", "--sample_file", *map(str, six), "--ksize", "31", "--outdir", str(out), "--num_threads", "2"]) == 0
        res[route] = out / "results"
        lines = [r.getMessage() for r in caplog.records if "panel pairs" in r.getMessage()]
        if lines:  # (the project's logger may not propagate to pytest's handler: the line is checked where it is seen)
            assert len(lines) == 1 and lines[0].startswith(f"{n_pairs} panel pairs: ")
            if route != "auto":
                assert f"{n_pairs} {route}" in lines[0] and f"0 {'dense' if route == 'sparse' else 'sparse'}" in lines[0]
    for name in FILES:
        assert _bytes(res["dense"] / name) == _bytes(res["sparse"] / name) == _bytes(res["auto"] / name), name


def test_compare_cohort_reports_the_route_of_every_panel_pair(hip_lib, six):
    plan = compare.check_inputs(list(map(str, six)), 31, str(six[0].parent), 2)
    n_hashes = [m[0] for m in plan["meta"]]
    runs = {}
    for route in ("dense", "sparse", "auto"):
        out = compare.compare_cohort(n_hashes, compare.file_loader(plan["paths"], 31, 2), budget=1, route=route)
        cells, self_rows, seconds = out  # (the tuple its callers unpack)
        assert [(p, q) for p, q, _, _ in out.routes] == [(p, q) for p in range(3) for q in range(p, 3)]
        assert route == "auto" or all(r == route for _, _, r, _ in out.routes)
        assert all(r in ("dense", "sparse") and (r == "sparse" or n == 0) for _, _, r, n in out.routes)
        runs[route] = (cells, self_rows)
    sparse = compare.compare_cohort(n_hashes, compare.file_loader(plan["paths"], 31, 2), budget=1, route="sparse")
    assert sum(n for _, _, _, n in sparse.routes) == int(np.triu(runs["sparse"][0]["n_shared"].astype(object), 1).sum())  # P is the shared hashes of the pairs
    for route in ("sparse", "auto"):
        assert runs[route][0].tobytes() == runs["dense"][0].tobytes() and runs[route][1].tobytes() == runs["dense"][1].tobytes()


def test_cohort_run_writes_the_same_residual_table_on_both_routes(hip_lib, trained, tmp_path, monkeypatch):  # noqa: F811
    tmp, cfg, files = trained
    monkeypatch.delenv(compare.PANEL_BYTES_ENV, raising=False)
    opts = ["--compare", "--residual", "--min_coverage_list", "0.05", "0.001"]
    res = {}
    for route in ("dense", "sparse"):
        monkeypatch.setenv(compare.ROUTE_ENV, route)
        out = tmp_path / route
        out.mkdir()
        assert cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(out), *opts]) == 0
        res[route] = out / "results"
    for name in FILES + [compare.RESIDUAL_TABLE_NAME]:
        assert _bytes(res["dense"] / name) == _bytes(res["sparse"] / name), name
