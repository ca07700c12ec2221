"""The cases of tests/compare_sparse_cases.py are what their names say (run lengths, chunk positions, the pair count two
independent ways); the header, the binding and the shared object agree on the sparse route's entries and constants; and
yh_compare_routed and the route word refuse bad input before any device work.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from compare_sparse_cases import CASES, K, LOG2, R, T8, expected, figures, hash_bits, sorted_records

from yacht_amd import _lib, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = sorted(n for n, c in CASES.items() if not c.get("closed_form"))


def _holders(case):
    """{hash: (kept holders in A, in B)} -- without keep bytes."""
    out = {}
    for side, xs in enumerate((case["a"], case["b"] or [])):
        for x in xs:
            for h in x.tolist():
                out.setdefault(h, [0, 0])[side] += 1
    return out


def test_every_sample_is_strictly_ascending_and_every_array_is_parallel():
    for name, case in CASES.items():
        for xs, abs_, keeps in ((case["a"], case["a_ab"], case["a_keep"]), (case["b"] or [], case["b_ab"], case["b_keep"])):
            for s, x in enumerate(xs):
                assert x.dtype == np.uint64 and (x.size < 2 or (x[1:] > x[:-1]).all()), (name, s)
                for other in (abs_, keeps):
                    assert other is None or other[s] is None or other[s].size == x.size, (name, s)


@pytest.mark.parametrize("name", SMALL)
def test_pair_count_two_ways(name):
    """P from the holders of every hash equals P from the oracle's cells: the n_shared of every cell the route sums
    (i < j in the symmetric call)."""
    case, fig = CASES[name], figures(CASES[name])
    cells = expected(name)[0]["n_shared"].astype(object)
    want = int(np.triu(cells, 1).sum()) if case["b"] is None else int(cells.sum())
    assert fig["n_pair_updates"] == want, name
    assert fig["pairs_sampled"] <= fig["n_pair_updates"]
    assert (fig["n_shared_hashes"] == 0) == (fig["n_pair_updates"] == 0) == (fig["longest_run"] == 0)


def test_cases_without_pairs():
    for name in ("no_shared", "all_empty_sym", "n_a_zero"):
        assert figures(CASES[name])["n_pair_updates"] == 0, name
    cells, self_a, _ = expected("no_shared")
    off = ~np.eye(self_a.size, dtype=bool)
    assert (cells.view(np.uint64).reshape(self_a.size, self_a.size, 4)[off] == 0).all() and (cells["n_shared"].diagonal() == self_a["n_kept"]).all()
    assert [x.size for x in CASES["one_empty_among_full"]["a"]].count(0) == 1 and figures(CASES["one_empty_among_full"])["longest_run"] == 4
    assert len(CASES["n_a_zero"]["a"]) == 0 and len(CASES["n_a_zero"]["b"]) == 2


def test_run_lengths():
    assert R >= 3 and K % 256 == 0
    for c in (2, R - 1, R, R + 1):
        case = CASES[f"run_sym_{c}"]
        counts = sorted(v[0] for v in _holders(case).values())
        assert counts[-1] == c and counts.count(1) > 10 * counts.count(2) > 0, c  # the runs sit among singletons
        assert figures(case)["longest_run"] == c
    n = 2 * T8 + 1
    assert len(CASES["run_sym_all"]["a"]) == n and figures(CASES["run_sym_all"])["longest_run"] == n
    big = CASES["run_4096"]
    m = _lib.YH_COMPARE_MAX_SAMPLES
    assert len(big["a"]) == len(big["b"]) == m and all(x.size == 2 for x in big["a"] + big["b"])
    fig = figures(big)
    assert (fig["n_shared_hashes"], fig["n_pair_updates"], fig["longest_run"]) == (1, m * m, 2 * m)
    assert np.intersect1d(np.concatenate(big["a"]), np.concatenate(big["b"])).size == 1  # the closed form: one hash a cell


def test_rectangular_cases():
    h = _holders(CASES["rect_1_by_R1_and_ca0"])
    assert [1, R + 1] in h.values() and [0, R + 2] in h.values()
    fig = figures(CASES["rect_1_by_R1_and_ca0"])
    assert (fig["n_shared_hashes"], fig["n_pair_updates"], fig["longest_run"]) == (1, R + 1, R + 2)  # the run of c_a = 0 gives nothing
    same, ref = CASES["rect_same_as_sym"], CASES["rect_same_as_sym_ref"]
    assert all(x is not y and np.array_equal(x, y) for x, y in zip(same["a"], same["b"])) and ref["b"] is None
    for x, y in zip(expected("rect_same_as_sym"), expected("rect_same_as_sym_ref")):
        assert np.array_equal(x, y)
    ld = CASES["rect_ld"]
    assert (len(ld["a"]), len(ld["b"]), ld["ld_extra"]) == (T8 + 1, T8 - 1, 3)


def _runs(case):
    """(first record, length) of every run of two or more in the sorted records."""
    rec = sorted_records(case)
    heads = np.flatnonzero(np.concatenate([[True], rec[1:] != rec[:-1]]))
    lens = np.diff(np.concatenate([heads, [rec.size]]))
    return rec.size, [(int(p), int(n)) for p, n in zip(heads, lens) if n > 1]


def test_chunk_edges():
    total, runs = _runs(CASES["chunk_first_is_last_of_0"])
    assert total > 2 * K and runs == [(K - 1, 3)]
    total, runs = _runs(CASES["chunk_last_is_first_of_1"])
    assert total > 2 * K and runs == [(K - 2, 3)]
    total, runs = _runs(CASES["chunk_straddles_1_2"])
    assert total > 2 * K and runs == [(2 * K - 2, 5)]
    total, runs = _runs(CASES["chunk_twos_both_sides"])
    assert total > 2 * K and runs == [(K - 2, 2), (K, 2), (2 * K - 2, 2), (2 * K, 2)]
    for name in ("chunk_first_is_last_of_0", "chunk_last_is_first_of_1", "chunk_straddles_1_2", "chunk_twos_both_sides"):
        runs = _runs(CASES[name])[1]
        fig = figures(CASES[name])
        assert fig["n_pair_updates"] == sum(n * (n - 1) // 2 for _, n in runs) and fig["n_shared_hashes"] == len(runs), name


def test_hash_range_cases():
    h = _holders(CASES["extremes_64"])
    assert h[0][0] == 3 and h[2 ** 64 - 1][0] == 3 and hash_bits(CASES["extremes_64"]) == 64
    narrow = CASES["narrow_42"]
    assert hash_bits(narrow) == narrow["bits"] == 42 and _holders(narrow)[2 ** 42 - 1] == [3, 2]
    fig = figures(narrow)
    assert 0 < fig["pairs_sampled"] < fig["n_pair_updates"]  # the window of 2^36 holds some of the shared hashes, not the topmost
    tiny = CASES["tiny_bits"]
    assert hash_bits(tiny) <= LOG2 and figures(tiny)["pairs_sampled"] == figures(tiny)["n_pair_updates"] > 0


def test_keep_cases():
    c = CASES["keep_kept_in_a_dropped_in_b"]
    assert np.array_equal(c["a"][0], c["b"][0]) and figures(c)["n_pair_updates"] == 0 and figures(c)["n_entries"] == c["a"][0].size
    c = CASES["keep_dropped_inside_run"]
    fig = figures(c)
    assert fig["longest_run"] == 4 and fig["n_pair_updates"] == 6  # six holders, the second and the fourth dropped
    assert figures(CASES["keep_none_kept"])["n_entries"] == 0
    for name, pair in (("keep_mask_known", (0x80, 0x80)), ("keep_mask_set0", (1, 0)), ("keep_mask_set0_sym", (1, 0)), ("keep_on_b_only", (1, 0))):
        c = CASES[name]
        assert (c["keep_and"], c["keep_eq"]) == pair
        full = sum(x.size for x in c["a"]) + (0 if c["b"] is None else sum(x.size for x in c["b"]))
        assert 0 < figures(c)["n_entries"] < full and figures(c)["n_pair_updates"] > 0, name
    assert CASES["keep_on_b_only"]["a_keep"] is None


def test_sum_cases():
    for name, cell in (("dot_carry_sym", (0, 2)), ("dot_carry_rect", (0, 1))):
        c = expected(name)[0][cell]
        assert c["dot_hi"] >= 1 and c["n_shared"] >= 3, name  # the product sum passes 2^64
    assert CASES["abund_on_a_only"]["b_ab"] is None and CASES["abund_on_a_only"]["a_ab"] is not None
    for name in ("abund_none_rect", "abund_none_sym"):
        cells = expected(name)[0]
        assert CASES[name]["a_ab"] is None and np.array_equal(cells["n_shared"], cells["sum_min"]) and np.array_equal(cells["n_shared"], cells["dot_lo"])


# ---- header, binding, shared object ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    with open(os.path.join(ROOT, "include", "yacht_hip.h")) as f:
        text = f.read()
    assert "#define YH_ABI_VERSION 8\n" in text
    lib = _lib.load()
    for name, n_args in (("yh_compare_sparse_work_bytes", 4), ("yh_compare_sparse_device", 23), ("yh_compare_routed", 19),
                         ("yh_compare_sparse_count_device", 17)):
        assert re.search(r"\b%s\(" % name, text), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), name
    for name, value in (("YH_COMPARE_RUN_SMALL", R), ("YH_COMPARE_SPARSE_CHUNK", K), ("YH_COMPARE_SAMPLE_LOG2", LOG2)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    for name, value in (("DENSE", 0), ("SPARSE", 1), ("AUTO", 2)):
        assert re.search(r"#define YH_COMPARE_ROUTE_%s +%d\b" % (name, value), text) and getattr(_lib, "YH_COMPARE_ROUTE_" + name) == value
    fields = [f for f, _ in _lib.CompareSparseInfo._fields_]
    declared = re.search(r"typedef struct yh_compare_sparse_info \{(.*?)\} yh_compare_sparse_info;", text, re.S).group(1)
    assert re.findall(r"uint(?:64|32)_t (\w+);", declared) == fields
    assert C.sizeof(_lib.CompareSparseInfo) == 6 * 8 + 2 * 4
    with open(os.path.join(ROOT, "yacht_amd", "build.py")) as f:
        assert '"yh_compare_sparse.hip"' in f.read()


# ---- refusals: all before any device work (this machine may have no device at all) ---------------------------------------------
def _refused(code, a, b=None, **kw):
    with pytest.raises(_lib.YachtHipError) as err:
        compare.compare_packed(a, b, **kw)
    assert err.value.code == code, str(err.value)
    return str(err.value)


def test_routed_refuses_before_device_work():
    lib = _lib.load()
    good = compare.pack([np.array([1, 2, 3], np.uint64), np.array([2, 9], np.uint64)])
    unsorted = compare.pack([np.array([1, 2, 3], np.uint64), np.array([9, 2], np.uint64)])
    for route in ("dense", "sparse", "auto"):
        assert "sample 1 of A" in _refused(_lib.YH_ERR_UNSORTED, unsorted, route=route)
        assert "of B" in _refused(_lib.YH_ERR_UNSORTED, good, unsorted, route=route)
        for bad in (np.array([0, 3, 2, 5], np.uint64), np.array([1, 3, 5, 5], np.uint64)):  # descending; not from 0
            _refused(_lib.YH_ERR_INVALID_ARG, (good[0], bad, None, None), good, route=route)
        many = (np.zeros(0, np.uint64), np.zeros(_lib.YH_COMPARE_MAX_SAMPLES + 2, np.uint64), None, None)
        _refused(_lib.YH_ERR_INVALID_ARG, many, route=route)
        _refused(_lib.YH_ERR_INVALID_ARG, good, good, ld_cells=1, route=route)
    # a route outside 0 .. 2, straight at the entry: refused before the samples are even looked at
    p = lambda arr: C.c_void_p(arr.ctypes.data)  # noqa: E731
    cells, selfs = np.zeros((2, 2), compare.CELL_DTYPE), np.zeros(2, compare.SELF_DTYPE)
    for route in (-1, 3, 7):
        rc = lib.yh_compare_routed(p(good[0]), p(good[1]), None, None, 2, p(good[0]), p(good[1]), None, None, 2, 0, 0, 0, p(cells), 2,
                                   p(selfs), p(selfs), route, None)
        assert rc == _lib.YH_ERR_INVALID_ARG, route


def test_route_word(monkeypatch):
    good = compare.pack([np.array([1, 2, 3], np.uint64)])
    monkeypatch.delenv(compare.ROUTE_ENV, raising=False)
    assert compare.route_code(None) == _lib.YH_COMPARE_ROUTE_AUTO
    for word, code in (("auto", 2), ("dense", 0), ("sparse", 1), ("Sparse", 1)):
        monkeypatch.setenv(compare.ROUTE_ENV, word)
        assert compare.route_code(None) == code
    monkeypatch.setenv(compare.ROUTE_ENV, "fast")
    for call in (lambda: compare.compare_packed(good), lambda: compare.compare([np.array([1], np.uint64)]),
                 lambda: compare.compare_cohort([3], lambda panel: ([good[0]], None, None))):
        with pytest.raises(ValueError, match="auto, dense, sparse"):
            call()
    with pytest.raises(ValueError, match="auto, dense, sparse"):
        compare.compare_packed(good, route="quick")


def test_sparse_work_bytes_and_device_form_refusals():
    m = _lib.YH_COMPARE_MAX_SAMPLES
    assert compare.sparse_work_bytes(m + 1, 1, 0, 0) == 0 and compare.sparse_work_bytes(1, m + 1, 0, 0) == 0
    assert compare.sparse_work_bytes(2, 2, 2 ** 31, 0) == 0 and compare.sparse_work_bytes(2, 2, 2 ** 30, 2 ** 30) == 0
    fake = 0x1000  # never dereferenced: every refusal comes first
    args = dict(d_a=fake, d_a_off=fake, d_a_abund=0, d_a_keep=0, n_a=2, total_a=6000, d_b=fake + 8, d_b_off=fake, d_b_abund=0, d_b_keep=0,
                n_b=2, total_b=6000, keep_and=0, keep_eq=0, d_cells=fake, ld_cells=2, d_self_a=fake, d_self_b=fake, d_work=fake,
                n_work_bytes=1 << 20, stream=0, hash_bits=64, d_info=0)
    for change in (dict(ld_cells=1), dict(d_a_off=0), dict(n_a=m + 1), dict(d_cells=0), dict(hash_bits=0), dict(hash_bits=65),
                   dict(total_a=2 ** 31), dict(total_a=2 ** 30, total_b=2 ** 30)):
        with pytest.raises(_lib.YachtHipError) as err:
            compare.compare_sparse_device(**{**args, **change})
        assert err.value.code == _lib.YH_ERR_INVALID_ARG, (change, str(err.value))
