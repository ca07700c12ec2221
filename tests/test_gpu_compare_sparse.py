"""The sparse route of the compare pass on the device: every case of tests/compare_cases.py and tests/compare_sparse_cases.py
through yh_compare_routed (sparse, dense, auto) and through yh_compare_sparse_device on torch buffers, exact equality with
the numpy oracle for every cell and self row and with the oracle's figures for yh_compare_sparse_info; the symmetric call
against the rectangular one and its transpose; nothing written behind n_b; nothing stale after a larger call; the same
bytes twice.  No test asserts which route `auto` picks: its constants are measured."""
import compare_cases
import compare_sparse_cases
import numpy as np
import pytest
from compare_sparse_cases import figures, hash_bits

from yacht_amd import _lib, compare

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
CASES = {**compare_cases.CASES, **compare_sparse_cases.CASES}
assert len(CASES) == len(compare_cases.CASES) + len(compare_sparse_cases.CASES)
INFO_FIELDS = ("n_entries", "n_shared_hashes", "n_pair_updates", "longest_run", "dense_steps")


def expected(name):
    return compare_sparse_cases.expected(name) if name in compare_sparse_cases.CASES else compare_cases.expected(name)


def _packed(case):
    a = compare.pack(case["a"], case["a_ab"], case["a_keep"])
    b = None if case["b"] is None else compare.pack(case["b"], case["b_ab"], case["b_keep"])
    return a, b


def _host(case, route, pad=0):
    """The host form.  Returns ((cells [n_a, n_b], self_a, self_b), info); with pad, the cells go into a poisoned buffer
    whose columns behind n_b must come back untouched."""
    a, b = _packed(case)
    n_a, n_b = a[1].size - 1, (a if b is None else b)[1].size - 1
    kw = {}
    if pad:
        kw = dict(ld_cells=n_b + pad, cells=np.full((n_a, n_b + pad, 4), SENTINEL, dtype=np.uint64).view(compare.CELL_DTYPE).reshape(n_a, n_b + pad))
    res = compare.compare_packed(a, b, case["keep_and"], case["keep_eq"], route=route, **kw)
    cells = res[0]
    if pad:
        assert (cells[:, n_b:].view(np.uint64) == SENTINEL).all(), "written behind n_b"
        cells = cells[:, :n_b]
    return (cells, res[1], res[2]), res.info


class _Dev:
    """One side on the device: the packed arrays as torch tensors (uint64 as int64 bits)."""

    def __init__(self, torch, packed):
        values, offsets, ab, keep = packed
        up = lambda arr, view: None if arr is None else torch.from_numpy(np.ascontiguousarray(arr).view(view).copy()).cuda()  # noqa: E731
        self.n, self.total = offsets.size - 1, int(offsets[-1])
        self.values, self.offsets = up(values, np.int64), up(offsets, np.int64)
        self.ab, self.keep = up(ab, np.int32), up(keep, np.uint8)
        self.selfs = torch.full((max(self.n, 1), 4), SENTINEL, dtype=torch.int64, device="cuda")

    def ptrs(self):
        p = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
        return p(self.values), self.offsets.data_ptr(), p(self.ab), p(self.keep)


def _device(case, bits=64, pad=0, cells=None, work=None):
    """yh_compare_sparse_device on the default stream.  Returns ((cells, self_a, self_b), info) as _host does."""
    import torch

    a, b = _packed(case)
    da = _Dev(torch, a)
    db = da if b is None else _Dev(torch, b)
    ld = db.n + pad
    if cells is None:
        cells = torch.full((max(da.n, 1), max(ld, 1), 4), SENTINEL, dtype=torch.int64, device="cuda")
    need = compare.sparse_work_bytes(da.n, db.n, da.total, db.total)
    assert need > 0
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert work.numel() >= need
    d_info = torch.full((7,), SENTINEL, dtype=torch.int64, device="cuda")
    compare.compare_sparse_device(*da.ptrs(), da.n, da.total, *db.ptrs(), db.n, db.total, case["keep_and"], case["keep_eq"],
                                  cells.data_ptr(), ld, da.selfs.data_ptr(), db.selfs.data_ptr(), work.data_ptr(), work.numel(), 0,
                                  bits, d_info.data_ptr())
    torch.cuda.synchronize()
    got = cells.cpu().numpy().view(np.uint64)[:da.n, :ld].copy().view(compare.CELL_DTYPE).reshape(da.n, ld)
    if pad:
        assert (got[:, db.n:].view(np.uint64) == SENTINEL).all(), "written behind n_b"
        got = got[:, :db.n]
    selfs = [d.selfs.cpu().numpy().view(np.uint64)[:d.n].copy().view(compare.SELF_DTYPE).reshape(d.n) for d in (da, db)]
    raw = d_info.cpu().numpy().view(np.uint64)
    info = dict(zip(INFO_FIELDS + ("pairs_sampled",), (int(x) for x in raw[:6])), route=int(raw[6]) & 0xFFFFFFFF, estimated=int(raw[6]) >> 32)
    return (got, selfs[0], selfs[1]), info


def _assert_equal(got, want, what):
    for g, w, part in zip(got, want, ("cells", "self_a", "self_b")):
        assert g.shape == w.shape, (what, part, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:5]
            raise AssertionError((what, part, [(tuple(ix), g[tuple(ix)], w[tuple(ix)]) for ix in bad]))


def _assert_info(info, fig, what):
    assert {f: info[f] for f in INFO_FIELDS} == {f: fig[f] for f in INFO_FIELDS}, what


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_oracle_on_the_sparse_route_in_both_forms(hip_lib, name):
    case, want, fig = CASES[name], expected(name), figures(CASES[name])
    pad = case.get("ld_extra", 0)
    got, info = _host(case, "sparse", pad)
    _assert_equal(got, want, (name, "host form, sparse"))
    _assert_info(info, fig, (name, "host form"))
    assert info["route"] == "sparse" and info["estimated"] == 0 and info["pairs_sampled"] == 0
    dense, d_info = _host(case, "dense", pad)
    _assert_equal(got, dense, (name, "sparse against dense"))
    assert d_info["route"] == "dense" and d_info["n_pair_updates"] == 0 and d_info["dense_steps"] == fig["dense_steps"]
    for bits in sorted({64, case.get("bits", hash_bits(case))}):
        got, info = _device(case, bits, pad)
        _assert_equal(got, want, (name, "device form", bits))
        if len(case["a"]) + len(case["a"] if case["b"] is None else case["b"]):
            _assert_info(info, fig, (name, "device form", bits))
            assert info["route"] == _lib.YH_COMPARE_ROUTE_SPARSE


@pytest.mark.parametrize("name", sorted(CASES))
def test_auto_fills_the_same_matrix_and_reports_its_sample(hip_lib, name):
    case, want, fig = CASES[name], expected(name), figures(CASES[name])
    got, info = _host(case, "auto", case.get("ld_extra", 0))
    _assert_equal(got, want, (name, "auto"))
    assert info["route"] in ("dense", "sparse") and info["dense_steps"] == fig["dense_steps"]
    assert info["pairs_sampled"] == fig["pairs_sampled"], name
    if info["route"] == "sparse":
        _assert_info(info, fig, (name, "auto took the sparse route"))
    else:
        assert info["n_pair_updates"] == 0


SYMMETRIC = sorted(n for n, c in CASES.items() if c["b"] is None)


@pytest.mark.parametrize("name", SYMMETRIC)
def test_symmetric_call_equals_the_rectangular_call_and_its_transpose(hip_lib, name):
    case = CASES[name]
    rect = dict(case, b=[x.copy() for x in case["a"]], b_ab=case["a_ab"], b_keep=case["a_keep"])
    for form in (lambda c: _device(c)[0], lambda c: _host(c, "sparse")[0]):
        sym, s_a, s_b = form(case)
        full, r_a, r_b = form(rect)
        assert np.array_equal(sym, full) and np.array_equal(sym, sym.T), name
        assert np.array_equal(s_a, r_a) and np.array_equal(s_a, s_b) and np.array_equal(r_a, r_b)
        i = np.arange(s_a.size)  # cell (i, i) agrees with self row i
        for c_f, s_f in (("n_shared", "n_kept"), ("sum_min", "sum"), ("dot_lo", "sq_lo"), ("dot_hi", "sq_hi")):
            assert np.array_equal(sym[c_f][i, i], s_a[s_f]), (name, c_f)


@pytest.mark.parametrize("name", ["rect_ld", f"tile_rect_{compare_cases.T + 1}x{compare_cases.T - 1}", "tile_sym_1", "abund_none_sym", "all_empty"])
def test_nothing_is_written_behind_n_b(hip_lib, name):
    case, want = CASES[name], expected(name)
    _assert_equal(_device(case, pad=3)[0], want, (name, "device"))
    _assert_equal(_host(case, "sparse", pad=3)[0], want, (name, "host"))


def test_a_large_call_followed_by_a_small_one_leaves_nothing_stale(hip_lib):
    """The same cell and work buffers for a call of three chunks with long lists of runs, then for small ones."""
    import torch

    big = CASES["windows_4_rect"]
    work = torch.full((compare.sparse_work_bytes(2, 2, 6000, 6000) + (1 << 16),), 0xFF, dtype=torch.uint8, device="cuda")
    cells = torch.full((64, 64, 4), SENTINEL, dtype=torch.int64, device="cuda")
    _assert_equal(_device(big, cells=cells.view(-1)[:2 * 2 * 4].view(2, 2, 4), work=work)[0], expected("windows_4_rect"), "large")
    for name in ("keep_nothing", "tile_rect_1x1", "run_sym_33", "no_shared", "keep_dropped_inside_run", "all_empty", "abund_none_rect"):
        want = expected(name)
        n_a, n_b = want[1].size, want[2].size
        view = cells.view(-1)[:n_a * n_b * 4].view(n_a, n_b, 4)
        got, info = _device(CASES[name], cells=view, work=work)
        _assert_equal(got, want, ("small after large", name))
        if n_a + n_b:
            _assert_info(info, figures(CASES[name]), ("small after large", name))


@pytest.mark.parametrize("name", ["panel_sym", "windows_8", "abund_max_on_three", "keep_known", "run_sym_33", "dot_carry_sym"])
def test_two_identical_calls_give_identical_bytes(hip_lib, name):
    for form in (lambda c: _device(c)[0], lambda c: _host(c, "sparse")[0], lambda c: _host(c, "auto")[0]):
        first, second = form(CASES[name]), form(CASES[name])
        for x, y in zip(first, second):
            assert x.tobytes() == y.tobytes(), name


@pytest.mark.parametrize("name", ["run_sym_33", "chunk_straddles_1_2", "rect_1_by_R1_and_ca0", "keep_dropped_inside_run", "keep_nothing", "narrow_42",
                                  "windows_4_rect", "all_empty"])
def test_the_grouping_alone_reports_the_same_figures(hip_lib, name):
    """yh_compare_sparse_count_device -- records, sort, runs, no matrix -- against the oracle's figures."""
    import torch

    case, fig = CASES[name], figures(CASES[name])
    a, b = _packed(case)
    da = _Dev(torch, a)
    db = da if b is None else _Dev(torch, b)
    work = torch.empty(compare.sparse_work_bytes(da.n, db.n, da.total, db.total), dtype=torch.uint8, device="cuda")
    d_info = torch.full((7,), SENTINEL, dtype=torch.int64, device="cuda")
    pa, pb = da.ptrs(), db.ptrs()
    for bits in sorted({64, case.get("bits", hash_bits(case))}):
        compare.sparse_count_device(pa[0], pa[1], pa[3], da.n, da.total, pb[0], pb[1], pb[3], db.n, db.total, case["keep_and"], case["keep_eq"],
                                    work.data_ptr(), work.numel(), 0, bits, d_info.data_ptr())
        torch.cuda.synchronize()
        raw = d_info.cpu().numpy().view(np.uint64)
        _assert_info(dict(zip(INFO_FIELDS, (int(x) for x in raw[:5]))), fig, (name, bits))
