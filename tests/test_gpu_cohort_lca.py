"""`yacht run --lineages --lineages_rank RANK` over a cohort, on the GPU: the block's lineage counts on the device
(yh_lca_batch_device + yh_lca_rows_pack_device in cohort._Device) against what they must equal.

From files: every results/<stem>/lca_summary.tsv of the fixture cohort of tests/test_gpu_cohort.py equals, byte for byte, the
file a single-sample run of that sample writes with the same options; results/cohort_lca.tsv holds, per sample, the
not_in_database row, the above_rank row and the taxa at the rank with the values of that sample's lca_summary.tsv, and the
three add up to the sample; the cohort by default and under YACHT_COHORT_LCA=loop, each in a fresh child process, leave the
same results/ tree; a row capacity of 1 takes the second pack and leaves the same files.  At the level of cohort._Device: the
rows collect() returns equal RefDB.lca of every sample, over two blocks and with a capacity that is too small."""
import json
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pandas as pd
import pytest
from test_gpu_cohort import trained as fixture_cohort  # noqa: F401  (the module's fixture, made again for this module)
from test_gpu_cohort_residual_device import _same_tree, _synthetic

from yacht_amd import cli, cohort, sigio, taxonomy
from yacht_amd.engine import LCA_ROW_DTYPE, RefDB
from yacht_amd.hypothesis_recovery_src import hyp_test_native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK = "genus"
COVS = ["--min_coverage_list", "1", "0.05", "0.001"]


def _lineage_file(cfg, path):
    """A small lineage table over the trained manifest, by position: two phyla, families of four, genera of two, every third
    organism named down to the species, one in eight at its genus only, one in ten without a lineage."""
    names = pd.read_csv(json.load(open(cfg))["manifest_file_path"], sep="\t")["organism_name"].tolist()
    assert len(names) >= 10
    with open(path, "w") as f:
        f.write("ident," + ",".join(taxonomy.RANKS) + "\n")
        for j, name in enumerate(names):
            if j % 10 == 9:
                continue
            lin = ["Bacteria", f"P{j % 2}", f"C{j % 2}", f"O{j % 2}", f"F{j % 2}_{j // 4}", f"G{j // 2}"]
            if j % 8 != 7:
                lin.append(f"G{j // 2} s{j if j % 3 == 0 else j // 2}")
            f.write(",".join([str(name).split()[0]] + lin + [""] * (len(taxonomy.RANKS) - len(lin))) + "\n")
    return ["--lineages", str(path), "--lineages_rank", RANK]


def _run(cfg, files, outdir, *opts):
    outdir.mkdir()
    assert cli.main(["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(outdir), *opts]) == 0
    return outdir / "results"


def _read(path):
    return pd.read_csv(path, sep="\t", float_precision="round_trip", keep_default_na=False)


def _check_cohort_table(res, files):
    """cohort_lca.tsv against the samples' own lca_summary.tsv files and sketches."""
    table = _read(res / taxonomy.COHORT_NAME)
    assert list(table.columns) == taxonomy.COHORT_COLUMNS
    stems = [cohort.sample_stem(str(f)) for f in files]
    assert list(dict.fromkeys(table["sample"])) == stems  # every sample, in cohort order
    at = taxonomy.RANKS.index(RANK) + 1
    n_taxa = 0
    for f, stem in zip(files, stems):
        mh = sigio.load_file_as_signatures(str(f), ksize=31)[0].minhash
        n_hashes = len(mh)
        total = n_hashes if mh.abundances is None else int(np.asarray(mh.abundances, dtype=np.uint64).sum())
        part = table[table["sample"] == stem].reset_index(drop=True)
        assert int(part["num_hashes_clade"].sum()) == n_hashes and int(part["abund_clade"].sum()) == total, stem
        if not (res / stem).exists():  # no overlap: its not_in_database row alone
            assert part["lineage"].tolist() == [taxonomy.NOT_IN_DATABASE] and part["f_hashes_clade"].tolist() == [1.0], stem
            continue
        assert part["lineage"].tolist()[:2] == [taxonomy.NOT_IN_DATABASE, taxonomy.ABOVE_RANK], stem
        summary = _read(res / stem / taxonomy.SUMMARY_NAME)
        none = summary[summary["rank"] == taxonomy.NOT_IN_DATABASE].iloc[0]
        assert part.loc[0, "num_hashes_clade"] == none["num_hashes_clade"] and part.loc[0, "abund_clade"] == none["abund_clade"], stem
        shallow = summary[(summary["rank"] != taxonomy.NOT_IN_DATABASE) & (summary["lineage"].map(lambda s: len(s.split(";")) if s else 0) < at)]
        assert part.loc[1, "num_hashes_clade"] == shallow["num_hashes_direct"].sum() and part.loc[1, "abund_clade"] == shallow["abund_direct"].sum(), stem
        want = summary[summary["rank"] == RANK].reset_index(drop=True)
        taxa = part.iloc[2:].reset_index(drop=True)
        assert taxa["lineage"].tolist() == want["lineage"].tolist(), stem
        for c in taxonomy.COHORT_COLUMNS[2:]:
            assert taxa[c].tolist() == want[c].tolist(), (stem, c)
        n_taxa += len(taxa)
    return n_taxa


@pytest.mark.parametrize("more", [[], ["--abundance", "--residual"]], ids=["plain", "abundance_residual"])
def test_fixture_cohort_equals_single_runs(hip_lib, fixture_cohort, tmp_path, more):  # noqa: F811
    tmp, cfg, files = fixture_cohort
    opts = _lineage_file(cfg, tmp_path / "lineages.csv") + COVS + more
    res = _run(cfg, files, tmp_path / "cohort", *opts)
    for f in files[:4]:
        stem = cohort.sample_stem(str(f))
        single = _run(cfg, [f], tmp_path / f"single_{stem}", *opts)  # (one file: the rank is accepted and ignored)
        assert (res / stem / taxonomy.SUMMARY_NAME).read_bytes() == (single / taxonomy.SUMMARY_NAME).read_bytes(), stem
        assert not (single / taxonomy.COHORT_NAME).exists()
        assert len(_read(single / taxonomy.SUMMARY_NAME)) >= 2  # (not_in_database and the root at the least)
    assert not (res / "none").exists()
    assert _check_cohort_table(res, files) >= 1  # (some sample has a taxon at the rank)


def test_the_default_and_the_loop_leave_the_same_tree(hip_lib, fixture_cohort, tmp_path):  # noqa: F811
    """Each in a fresh child process, side by side."""
    tmp, cfg, files = fixture_cohort
    opts = _lineage_file(cfg, tmp_path / "lineages.csv") + COVS + ["--abundance"]
    running = []
    for name, mode in (("device", None), ("loop", "loop")):
        outdir = tmp_path / name
        outdir.mkdir()
        env = {k: v for k, v in os.environ.items() if k != "YACHT_COHORT_LCA"}
        if mode is not None:
            env["YACHT_COHORT_LCA"] = mode
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        running.append(subprocess.Popen([sys.executable, "-m", "yacht_amd", "run", "--json", str(cfg), "--sample_file", *map(str, files),
                                         "--num_threads", "2", "--outdir", str(outdir), *opts], env=env, cwd=ROOT,
                                        stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    for child in running:
        _out, err = child.communicate()
        assert child.returncode == 0, err[-2000:]
    names = _same_tree(str(tmp_path / "device" / "results"), str(tmp_path / "loop" / "results"), "device against loop")
    assert taxonomy.COHORT_NAME in names and all(f"{cohort.sample_stem(str(f))}/{taxonomy.SUMMARY_NAME}" in names for f in files[:4])


def test_a_row_capacity_of_one_takes_the_second_pack(hip_lib, fixture_cohort, tmp_path, monkeypatch):  # noqa: F811
    tmp, cfg, files = fixture_cohort
    opts = _lineage_file(cfg, tmp_path / "lineages.csv") + COVS
    want = _run(cfg, files, tmp_path / "roomy", *opts)
    monkeypatch.setattr(cohort, "LCA_ROWS_CAP", 1)
    packed = []
    real = RefDB.lca_rows_pack_device
    monkeypatch.setattr(RefDB, "lca_rows_pack_device", lambda self, *a: (packed.append(a[3]), real(self, *a))[1])
    got = _run(cfg, files, tmp_path / "tight", *opts)
    assert len(packed) == 2 and packed[0] == 1 and packed[1] > 1  # the block's pack, then once more with room
    _same_tree(str(want), str(got), "capacity 1")


# ---- cohort._Device ----------------------------------------------------------------------------------------------------------
def _chain(n_refs):
    """A taxonomy of 40 nodes: a spine of five, then 35 children of the spine's end; reference j hangs at node j % 40."""
    parent = np.array([0, 0, 1, 2, 3] + [4] * 35, dtype=np.uint32)
    depth = np.array([0, 1, 2, 3, 4] + [5] * 35, dtype=np.uint8)
    return parent, depth, (np.arange(n_refs) % 40).astype(np.uint32)


def _check_block_lca(db, block, abunds, got, n_nodes, what):
    rows = got[-1]
    assert rows.dtype == LCA_ROW_DTYPE
    dense = np.zeros((len(block), n_nodes, 2), dtype=np.uint64)
    dense[rows["sample"], rows["node"], 0], dense[rows["sample"], rows["node"], 1] = rows["n_hashes"], rows["w_hashes"]
    assert (rows["n_hashes"] != 0).all() and len(set(zip(rows["sample"].tolist(), rows["node"].tolist()))) == rows.size
    order = rows["sample"].astype(np.int64) * n_nodes + rows["node"]
    assert (np.diff(order) > 0).all(), what  # ascending (sample, node)
    for s, sample in enumerate(block):
        want = db.lca(sample, None if abunds is None else abunds[s], want_nodes=False)[1]
        assert np.array_equal(dense[s], want), (what, s)
    return int(rows.size)


def test_device_blocks_against_the_single_call(hip_lib):
    """Two blocks back to back on one _Device, the second smaller; abundances for two samples in three; one sample without a
    hit and an empty one; then a _Device whose row buffer holds 64 rows."""
    values, offsets, samples, abunds = _synthetic(85)
    covs = [1.0, 0.1]
    with RefDB(values, offsets) as db:
        tree = _chain(db.n_refs)
        db.set_taxonomy(*tree)
        n_max = int(np.max(db.sizes))
        tab = hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), 31, 0.99, 0.95, 1.0)
        dev = cohort._Device(db, covs, 31, 0.95, tab[5], lca_nodes=40, max_samples=65)
        timer = defaultdict(float)
        for lo, hi in ((0, 65), (65, 85)):
            got = dev.collect(dev.launch(samples[lo:hi], None, abunds[lo:hi]), timer)
            assert len(got) == 5
            assert _check_block_lca(db, samples[lo:hi], abunds[lo:hi], got, 40, f"block {lo}") > 4 * (hi - lo)  # (eight organisms a sample)
        assert timer["lca_repacked_blocks"] == 0 and timer["gpu_lca"] > 0
        got = dev.collect(dev.launch(samples[:9]), timer)  # without abundances every hash counts once
        _check_block_lca(db, samples[:9], None, got, 40, "no abundances")
        assert np.array_equal(got[-1]["n_hashes"], got[-1]["w_hashes"])
        tight = cohort._Device(db, covs, 31, 0.95, tab[5], lca_nodes=40, lca_cap=64, max_samples=30)
        first = tight.collect(tight.launch(samples[:30], None, abunds[:30]), timer)
        k = _check_block_lca(db, samples[:30], abunds[:30], first, 40, "second pack")
        assert k > 64 and timer["lca_repacked_blocks"] == 1 and tight.l_cap > k
        second = tight.collect(tight.launch(samples[30:50], None, abunds[30:50]), timer)
        assert timer["lca_repacked_blocks"] == 1
        _check_block_lca(db, samples[30:50], abunds[30:50], second, 40, "room after growth")
