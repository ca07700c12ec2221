"""Everything of the compare pass that needs no device: the cases of tests/compare_cases.py hold what they are named for,
the header, the binding, the host form's refusals (they come before any device work), the metrics on hand values, the
writers' layouts and the commands' refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
from compare_cases import A_MAX, CASES, E, NARROW_BITS, T, U64_MAX, W, expected, windows_of

from yacht_amd import _lib, cli, compare, sigio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dot(c):
    return int(c["dot_lo"]) + (int(c["dot_hi"]) << 64)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def test_every_sample_is_strictly_ascending_and_every_array_is_parallel():
    for name, case in CASES.items():
        for side in ("a", "b"):
            if case[side] is None:
                assert side == "b"
                continue
            for s, x in enumerate(case[side]):
                assert x.dtype == np.uint64 and (x.size < 2 or (x[1:] > x[:-1]).all()), (name, side, s)
                for extra in (case[f"{side}_ab"], case[f"{side}_keep"]):
                    assert extra is None or extra[s] is None or extra[s].size == x.size, (name, side, s)


def test_tile_and_length_edges_are_all_there():
    sizes = (1, T - 1, T, T + 1, 2 * T + 1)
    for na in sizes:
        assert len(CASES[f"tile_sym_{na}"]["a"]) == na and CASES[f"tile_sym_{na}"]["b"] is None
        for nb in sizes:
            c = CASES[f"tile_rect_{na}x{nb}"]
            assert (len(c["a"]), len(c["b"])) == (na, nb)
            assert (expected(f"tile_rect_{na}x{nb}")[0]["n_shared"] > 0).mean() > 0.5
    lens = [x.size for x in CASES["lengths_rect"]["a"]]
    assert lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1]
    assert {0, 1, E - 1, E, E + 1} <= set(lens) and max(lens) > 3 * E
    assert [x.size for x in CASES["lengths_rect"]["b"]] == lens[::-1]
    cells, s_a, s_b = expected("lengths_rect")
    assert (cells["n_shared"][0] == 0).all() and (cells["n_shared"][:, 0] == 0).all() and s_a["n_kept"].tolist() == lens
    assert not expected("all_empty")[0].view(np.uint64).any()


def test_window_cases_take_the_paths_they_are_named_for():
    assert windows_of(CASES["windows_4_rect"]) == 4 and windows_of(CASES["windows_4_sym"]) == 4
    assert windows_of(CASES["windows_8"]) == 8 and windows_of(CASES["windows_64"]) == W == 64
    assert windows_of(CASES["window_boundaries_4"]) == 4 and windows_of(CASES["window_boundaries_8"]) == 8
    assert windows_of(CASES["narrow_range"]) == 4
    assert all(windows_of(CASES[n]) == 1 for n in CASES if n.startswith(("tile_", "lengths_", "abund_", "keep_", "panel_")))
    for n in ("window_boundaries_4", "window_boundaries_8"):
        both = np.intersect1d(CASES[n]["a"][0], CASES[n]["b"][0])
        for k in range(1, W, 7):  # on a boundary and just below it, shared by both sides
            assert ((k << 58) in both or ((k << 58) - 1) in both), (n, k)
        assert 0 in both and U64_MAX in both
    assert all(int(x.max()) < (1 << NARROW_BITS) for x in CASES["narrow_range"]["a"] + CASES["narrow_range"]["b"])
    assert (expected("narrow_range")[0]["n_shared"] > 500).all()
    top = (1 << NARROW_BITS) - 1  # the call's largest hash: its windows start at multiples of (top >> 2) + 1 = 2^40
    both = np.intersect1d(CASES["narrow_range"]["a"][0], CASES["narrow_range"]["b"][0])
    assert all(v in both for v in (top, 1 << 40, (1 << 40) - 1, 3 << 40, (3 << 40) - 1))
    c = CASES["consecutive_and_extremes"]
    assert c["a"][0].size > E and (np.diff(c["a"][0]) == 1).all() and int(c["a"][1][-1]) == U64_MAX and int(c["a"][2][0]) == 0
    cells = expected("consecutive_and_extremes")[0]["n_shared"]
    assert cells[0].tolist() == [500, 0, 1, 1] and cells[1].tolist() == [0, 700, 1, 0] and cells[2].tolist() == [0, 1, 2, 1]
    cells = expected("clustered_beside_uniform")[0]["n_shared"]
    assert cells[0, 0] == len(range(1000, 2000, 3)) and CASES["clustered_beside_uniform"]["a"][0].size > 7 * E


def test_set_relations():
    c, (cells, s_a, _s_b) = CASES["relations"], expected("relations")
    x, sub, dis, ends = c["a"]
    n = cells["n_shared"]
    assert n[0, 0] == x.size and _dot(cells[0, 0]) != _dot(cells[1, 1])  # identical hashes, abundances of their own
    assert n[0, 1] == sub.size == n[1, 0] and 0 < sub.size < x.size  # a strict subset
    assert n[0, 2] == 0 and n[2, 0] == 0 and n[1, 2] == 0 and dis.size > 100  # disjoint
    assert n[0, 3] == 2 and n[3, 0] == 2 and ends[0] == x[0] and ends[-1] == x[-1] and ends.size > 100  # first and last only


def test_abundance_cases():
    both, ones, none = expected("abund_both"), expected("abund_ones"), expected("abund_none")
    for got in (ones, none):  # abundance 1 everywhere is the unweighted count
        assert np.array_equal(got[0]["n_shared"], got[0]["sum_min"]) and np.array_equal(got[0]["n_shared"], got[0]["dot_lo"])
    assert all(np.array_equal(x, y) for x, y in zip(ones, none))
    assert np.array_equal(both[0]["n_shared"], none[0]["n_shared"]) and (both[0]["sum_min"] > none[0]["sum_min"]).all()
    a_only, b_only = expected("abund_a_only"), expected("abund_b_only")
    assert np.array_equal(a_only[0]["sum_min"], none[0]["sum_min"]) and (a_only[0]["dot_lo"] > none[0]["dot_lo"]).all()
    assert np.array_equal(a_only[1], both[1]) and np.array_equal(a_only[2], none[2]) and np.array_equal(b_only[2], both[2])
    big = expected("abund_max_on_three")[0][0, 0]
    assert int(big["dot_hi"]) >= 1 and int(big["sum_min"]) > 2 ** 32 and _dot(big) >= 3 * A_MAX * A_MAX
    sym = expected("abund_max_sym")
    assert (sym[1]["sq_hi"] >= 1).all() and int(sym[1]["sq_lo"][0]) + (int(sym[1]["sq_hi"][0]) << 64) == CASES["abund_max_sym"]["a"][0].size * A_MAX ** 2


def test_keep_cases():
    full = expected("abund_both")
    for name in ("keep_set0", "keep_set3", "keep_known", "keep_known_not_set0", "keep_a_only", "keep_b_only"):
        cells, s_a, s_b = expected(name)
        assert (cells["n_shared"] <= full[0]["n_shared"]).all() and 0 < cells["n_shared"].sum() < full[0]["n_shared"].sum(), name
    assert np.array_equal(expected("keep_a_only")[2], full[2]) and (expected("keep_a_only")[1]["n_kept"] < full[1]["n_kept"]).all()
    assert np.array_equal(expected("keep_b_only")[1], full[1]) and (expected("keep_b_only")[2]["n_kept"] < full[2]["n_kept"]).all()
    assert not any(part.view(np.uint64).any() for part in expected("keep_nothing"))
    cells, s_a, s_b = expected("keep_a_kept_b_dropped")
    assert cells["n_shared"][0, 0] == 0 and s_a["n_kept"][0] == 200 and s_b["n_kept"][0] == 200
    cells, s_a, _ = expected("keep_sym")
    i = np.arange(s_a.size)
    assert np.array_equal(cells["n_shared"][i, i], s_a["n_kept"]) and np.array_equal(cells, cells.T)


def test_the_panel_case():
    c, (cells, s_a, _s) = CASES["panel_sym"], expected("panel_sym")
    assert len(c["a"]) == 2 * T + 3 and all(20 <= x.size <= 60 for x in c["a"])
    off = ~np.eye(s_a.size, dtype=bool)
    assert (cells["n_shared"][off] > 0).mean() > 0.9


# ---- header and binding --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_abi_stays_8():
    with open(os.path.join(ROOT, "include", "yacht_hip.h")) as f:
        text = f.read()
    assert "#define YH_ABI_VERSION 8\n" in text
    for name in ("yh_compare_work_bytes", "yh_compare_device", "yh_compare"):
        assert re.search(r"\b%s\(" % name, text), name
    for name, value in (("YH_COMPARE_TILE", T), ("YH_COMPARE_SLICE", E), ("YH_COMPARE_MAX_WINDOWS", W),
                        ("YH_COMPARE_MAX_SAMPLES", _lib.YH_COMPARE_MAX_SAMPLES)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    for field in ("n_shared", "sum_min", "dot_lo", "dot_hi", "n_kept", "sq_lo", "sq_hi"):
        assert re.search(r"uint64_t %s;" % field, text), field
    assert "typedef struct yh_compare_cell" in text and "typedef struct yh_compare_self" in text
    assert _lib.YH_COMPARE_MAX_SAMPLES ** 2 * 32 <= 512 << 20  # a maximal call's matrix: a few hundred MB at most


def test_binding_types_the_entries():
    assert [len(_lib.SIGNATURES[n][1]) for n in ("yh_compare_work_bytes", "yh_compare_device", "yh_compare")] == [4, 21, 17]
    assert _lib.SIGNATURES["yh_compare_work_bytes"][0] is C.c_uint64
    assert C.sizeof(_lib.CompareCell) == 32 == compare.CELL_DTYPE.itemsize and C.sizeof(_lib.CompareSelf) == 32 == compare.SELF_DTYPE.itemsize
    assert compare.CELL_DTYPE.names == tuple(f for f, _ in _lib.CompareCell._fields_)
    assert compare.SELF_DTYPE.names == tuple(f for f, _ in _lib.CompareSelf._fields_)
    with open(os.path.join(ROOT, "yacht_amd", "build.py")) as f:
        assert '"yh_compare.hip"' in f.read()


# ---- the host form's refusals: all before any device work (this machine may have no device at all) ----------------------------
def _refused(code, a, b=None, **kw):
    with pytest.raises(_lib.YachtHipError) as err:
        compare.compare_packed(a, b, **kw)
    assert err.value.code == code, str(err.value)
    return str(err.value)


def test_host_form_refuses_before_device_work():
    lib = _lib.load()
    assert lib.yh_abi_version() == 8
    good = compare.pack([np.array([1, 2, 3], np.uint64), np.array([2, 9], np.uint64)])
    unsorted = compare.pack([np.array([1, 2, 3], np.uint64), np.array([9, 2], np.uint64)])
    equal = compare.pack([np.array([4, 4], np.uint64)])
    assert "sample 1 of A" in _refused(_lib.YH_ERR_UNSORTED, unsorted)
    assert "of B" in _refused(_lib.YH_ERR_UNSORTED, good, unsorted)
    _refused(_lib.YH_ERR_UNSORTED, equal, good)  # strictly ascending: an equal pair is refused too
    for bad in (np.array([0, 3, 2, 5], np.uint64), np.array([1, 3, 5, 5], np.uint64)):  # descending; not from 0
        _refused(_lib.YH_ERR_INVALID_ARG, (good[0], bad, None, None), good)
        _refused(_lib.YH_ERR_INVALID_ARG, good, (good[0], bad, None, None))
    many = (np.zeros(0, np.uint64), np.zeros(_lib.YH_COMPARE_MAX_SAMPLES + 2, np.uint64), None, None)
    assert str(_lib.YH_COMPARE_MAX_SAMPLES) in _refused(_lib.YH_ERR_INVALID_ARG, many)
    _refused(_lib.YH_ERR_INVALID_ARG, good, many)
    _refused(_lib.YH_ERR_INVALID_ARG, good, good, ld_cells=1)  # ld_cells < n_b
    assert compare.work_bytes(_lib.YH_COMPARE_MAX_SAMPLES + 1, 1, 0, 0) == 0 and compare.work_bytes(1, _lib.YH_COMPARE_MAX_SAMPLES + 1, 0, 0) == 0
    # one window needs no partial sums; several need the largest hash and a slab per tile and window
    assert compare.work_bytes(2 * T + 1, 2 * T + 1, 1000, 1000) == 256
    assert compare.work_bytes(2, 2, 6000, 6000) == 512 + 4 * 64 * 32
    assert compare.work_bytes(1, 1, 33000, 33000) == 512 + W * 64 * 32


def test_device_form_refuses_bad_arguments_before_any_launch():
    fake = 0x1000  # never dereferenced: every refusal comes first
    args = dict(d_a=fake, d_a_off=fake, d_a_abund=0, d_a_keep=0, n_a=2, total_a=6000, d_b=fake + 8, d_b_off=fake, d_b_abund=0, d_b_keep=0,
                n_b=2, total_b=6000, keep_and=0, keep_eq=0, d_cells=fake, ld_cells=2, d_self_a=fake, d_self_b=fake, d_work=fake,
                n_work_bytes=256, stream=0)
    for change in (dict(), dict(d_work=0, n_work_bytes=1 << 20), dict(ld_cells=1, n_work_bytes=1 << 20), dict(d_a_off=0, n_work_bytes=1 << 20),
                   dict(n_a=_lib.YH_COMPARE_MAX_SAMPLES + 1, n_work_bytes=1 << 20), dict(d_cells=0, n_work_bytes=1 << 20)):
        with pytest.raises(_lib.YachtHipError) as err:
            compare.compare_device(**{**args, **change})
        assert err.value.code == _lib.YH_ERR_INVALID_ARG, (change, str(err.value))


# ---- metrics -------------------------------------------------------------------------------------------------------------------
def _cells(rows):
    return np.array(rows, dtype=compare.CELL_DTYPE)


def test_metrics_on_hand_values():
    # A: 4 hashes, abundances 1 2 3 4; B: 2 hashes, abundances 2 2, both shared with A's 2 and 3
    cells = _cells([[(2, 4, 10, 0)]])
    s_a = np.array([(4, 10, 30, 0)], dtype=compare.SELF_DTYPE)
    s_b = np.array([(2, 4, 8, 0)], dtype=compare.SELF_DTYPE)
    m = compare.metrics(cells, s_a, s_b, 31)
    assert set(m) == set(compare.METRICS) and all(v.shape == (1, 1) and v.dtype == np.float64 for v in m.values())
    assert m["jaccard"][0, 0] == 2 / 4 and m["containment_a_in_b"][0, 0] == 0.5 and m["containment_b_in_a"][0, 0] == 1.0
    assert m["max_containment"][0, 0] == 1.0 and m["ani_max_containment"][0, 0] == 1.0
    assert m["bray_curtis"][0, 0] == 1 - 8 / 14
    cos = 10 / (math.sqrt(30) * math.sqrt(8))
    assert m["cosine"][0, 0] == pytest.approx(cos, rel=1e-15) and m["angular_similarity"][0, 0] == pytest.approx(1 - 2 * math.acos(cos) / math.pi, rel=1e-14)
    half = compare.metrics(_cells([[(1, 1, 1, 0)]]), s_b, s_b, 21)
    assert half["max_containment"][0, 0] == 0.5 and half["ani_max_containment"][0, 0] == 0.5 ** (1 / 21)


def test_metrics_with_zero_denominators():
    cells = _cells([[(0, 0, 0, 0), (0, 0, 0, 0)], [(0, 0, 0, 0), (3, 3, 3, 0)]])
    selfs = np.array([(0, 0, 0, 0), (3, 3, 3, 0)], dtype=compare.SELF_DTYPE)
    m = compare.metrics(cells, selfs, selfs, 31)
    for name in compare.METRICS:
        want = [[1.0, 1.0], [1.0, 0.0]] if name == "bray_curtis" else [[0.0, 0.0], [0.0, 1.0]]
        assert m[name].tolist() == want, name
    assert np.isfinite(np.concatenate([v.ravel() for v in m.values()])).all()


def test_metrics_take_a_128_bit_dot():
    # two samples of three hashes of abundance 2^32 - 1, all shared: dot = sq = 3 (2^32 - 1)^2 > 2^64, cosine exactly 1
    sq = 3 * A_MAX * A_MAX
    lo, hi = sq & U64_MAX, sq >> 64
    assert hi == 2
    cells = _cells([[(3, 3 * A_MAX, lo, hi)]])
    s = np.array([(3, 3 * A_MAX, lo, hi)], dtype=compare.SELF_DTYPE)
    m = compare.metrics(cells, s, s, 31)
    assert m["cosine"][0, 0] == pytest.approx(1.0, rel=1e-15) and m["angular_similarity"][0, 0] == pytest.approx(1.0, abs=1e-7)
    assert m["bray_curtis"][0, 0] == 0.0
    assert compare.wide(np.array([lo], np.uint64), np.array([hi], np.uint64))[0] == pytest.approx(float(sq), rel=1e-15)
    # a dot a quarter of the norms' product: 2^126 against sqrt(2^128) * sqrt(2^128)... as halves
    m = compare.metrics(_cells([[(1, 1, 0, 1 << 62)]]), np.array([(1, 1, 0, 1 << 63)], dtype=compare.SELF_DTYPE),
                        np.array([(1, 1, 0, 1 << 63)], dtype=compare.SELF_DTYPE), 31)
    assert m["cosine"][0, 0] == pytest.approx(0.5, rel=1e-15)  # (two square roots, a product and a quotient: four roundings of 2^-53)


# ---- writers -------------------------------------------------------------------------------------------------------------------
def test_writers_layouts(tmp_path):
    cells, s_a, _ = expected("panel_sym")
    cells, s_a = cells[:4, :4].copy(), s_a[:4].copy()
    stems = ["s0", "s1", "s2", "s3"]
    compare.write_outputs(str(tmp_path), stems, cells, s_a, 31)
    assert sorted(os.listdir(tmp_path)) == sorted([compare.TABLE_NAME] + [compare.MATRIX_NAME.format(m) for m in compare.MATRIX_METRICS])
    table = pd.read_csv(tmp_path / compare.TABLE_NAME, sep="\t", float_precision="round_trip")
    assert list(table.columns) == compare.TABLE_COLUMNS == ["sample_a", "sample_b", "n_hashes_a", "n_hashes_b", "n_shared", "jaccard",
                                                            "containment_a_in_b", "containment_b_in_a", "max_containment",
                                                            "ani_max_containment", "bray_curtis", "cosine", "angular_similarity", "abund_sum_min"]
    assert list(zip(table["sample_a"], table["sample_b"])) == [("s0", "s1"), ("s0", "s2"), ("s0", "s3"), ("s1", "s2"), ("s1", "s3"), ("s2", "s3")]
    m = compare.metrics(cells, s_a, s_a, 31)
    assert table["n_shared"].tolist() == [int(cells["n_shared"][i, j]) for i in range(4) for j in range(i + 1, 4)]
    assert table["n_hashes_a"].tolist() == [int(s_a["n_kept"][i]) for i in range(4) for j in range(i + 1, 4)]
    assert table["abund_sum_min"].tolist() == [int(cells["sum_min"][i, j]) for i in range(4) for j in range(i + 1, 4)]
    for name in compare.METRICS:
        assert table[name].tolist() == [float(m[name][i, j]) for i in range(4) for j in range(i + 1, 4)], name
    for name in compare.MATRIX_METRICS:
        with open(tmp_path / compare.MATRIX_NAME.format(name)) as f:
            lines = f.read().split("\n")
        assert lines[0] == "s0,s1,s2,s3" and len(lines) == 6 and lines[-1] == ""
        got = np.array([[float(x) for x in line.split(",")] for line in lines[1:5]])
        key = "containment_a_in_b" if name == "containment" else name
        off = ~np.eye(4, dtype=bool)
        assert np.array_equal(got[off], m[key][off]), name
        assert got.diagonal().tolist() == [0.0 if name == "bray_curtis" else pytest.approx(1.0, abs=1e-7)] * 4, name
        assert np.array_equal(got, got.T) == (name != "containment")
    # the diagonal comes from the self rows, whatever the cells hold there
    junk = cells.copy()
    junk["n_shared"][np.arange(4), np.arange(4)] = 0
    assert np.array_equal(compare.matrices(junk, s_a, 31)["jaccard"], compare.matrices(cells, s_a, 31)["jaccard"])


def test_panels_hold_two_samples_at_least_and_respect_the_limits():
    assert [list(p) for p in compare.plan_panels([100] * 6, 1)] == [[0, 1], [2, 3], [4, 5]]
    assert [list(p) for p in compare.plan_panels([100] * 5, 1)] == [[0, 1], [2, 3], [4]]
    assert [list(p) for p in compare.plan_panels([100] * 5, 100 * compare.BYTES_PER_HASH * 3)] == [[0, 1, 2], [3, 4]]
    assert [list(p) for p in compare.plan_panels([100] * 5, compare.PANEL_BYTES_DEFAULT)] == [[0, 1, 2, 3, 4]]
    big = compare.plan_panels([1] * (2 * _lib.YH_COMPARE_MAX_SAMPLES + 5), compare.PANEL_BYTES_DEFAULT)
    assert [len(p) for p in big] == [_lib.YH_COMPARE_MAX_SAMPLES, _lib.YH_COMPARE_MAX_SAMPLES, 5]
    assert compare.PANEL_BYTES_DEFAULT == 1 << 30 and compare.PANEL_BYTES_ENV == "YACHT_COMPARE_PANEL_BYTES"


# ---- the commands' refusals: before any device work, nothing written -----------------------------------------------------------
def _sig(path, mins, scaled=1000, ksize=31, abund=None):
    sigio.write_sig_zip([sigio.make_signature(np.asarray(mins, np.uint64), ksize=ksize, scaled=scaled, name=os.path.basename(str(path)),
                                              abundances=abund)], str(path))
    return str(path)


def test_command_refusals(tmp_path, monkeypatch):
    monkeypatch.setattr(compare, "compare_cohort", lambda *a, **k: pytest.fail("device work after a refusal"))
    out = tmp_path / "out"
    out.mkdir()
    one = _sig(tmp_path / "one.sig.zip", [1, 5, 9])
    two = _sig(tmp_path / "two.sig.zip", [1, 7], abund=[2, 3])
    coarse = _sig(tmp_path / "coarse.sig.zip", [1, 5], scaled=2000)
    other_k = _sig(tmp_path / "other_k.sig.zip", [1, 5], ksize=21)
    with pytest.raises(ValueError, match="two or more --sample_file"):
        cli.main(["run", "--json", str(tmp_path / "missing.json"), "--sample_file", one, "--compare", "--outdir", str(out)])
    with pytest.raises(ValueError, match="two or more --sample_file"):
        cli.main(["compare", "--sample_file", one, "--ksize", "31", "--outdir", str(out)])
    with pytest.raises(ValueError, match="scale factors differ"):
        cli.main(["compare", "--sample_file", one, two, coarse, "--ksize", "31", "--outdir", str(out)])
    with pytest.raises(ValueError, match="Expected exactly one signature with ksize 31"):
        cli.main(["compare", "--sample_file", one, other_k, "--ksize", "31", "--outdir", str(out)])
    bare = tmp_path / "bare.sig.zip"
    import zipfile

    with zipfile.ZipFile(bare, "w") as z:
        z.writestr("signatures/x.sig", "[]")
    with pytest.raises(FileNotFoundError, match="missing a manifest"):
        cli.main(["compare", "--sample_file", one, str(bare), "--ksize", "31", "--outdir", str(out)])
    with pytest.raises(ValueError, match="does not exist"):
        cli.main(["compare", "--sample_file", one, str(tmp_path / "absent.sig.zip"), "--ksize", "31", "--outdir", str(out)])
    twin = tmp_path / "sub"
    twin.mkdir()
    with pytest.raises(ValueError, match="share the name"):
        cli.main(["compare", "--sample_file", one, _sig(twin / "one.sig.zip", [2, 3]), "--ksize", "31", "--outdir", str(out)])
    assert os.listdir(out) == []
    plan = compare.check_inputs([one, two], 31, str(out))
    assert plan["stems"] == ["one", "two"] and [m[0] for m in plan["meta"]] == [3, 2] and plan["meta"][0][1] is None


def test_run_takes_the_flag():
    args = cli.build_parser().parse_args(["run", "--json", "x", "--sample_file", "a", "b", "--compare"])
    assert args.compare is True
    assert cli.build_parser().parse_args(["run", "--json", "x", "--sample_file", "a", "b"]).compare is False
    args = cli.build_parser().parse_args(["compare", "--sample_file", "a", "b", "--ksize", "21"])
    assert args.func is compare.main and args.ksize == 21
