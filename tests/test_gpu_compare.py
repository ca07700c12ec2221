"""yh_compare_device and yh_compare on the device against the numpy oracle of tests/compare_cases.py: every case through
both forms, exact equality of every cell and self row; the symmetric call against the rectangular one and its transpose;
nothing written outside the matrix; nothing stale after a larger call; the same bytes twice; and n_shared against the
overlap counts of the batched run step, which predates this pass."""
import numpy as np
import pytest
from compare_cases import CASES, T, expected, windows_of

from yacht_amd import compare
from yacht_amd.engine import RefDB

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A


def _packed(case):
    a = compare.pack(case["a"], case["a_ab"], case["a_keep"])
    b = None if case["b"] is None else compare.pack(case["b"], case["b_ab"], case["b_keep"])
    return a, b


def _host(case, **kw):
    a, b = _packed(case)
    return compare.compare_packed(a, b, case["keep_and"], case["keep_eq"], **kw)


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


def _device(case, pad=0, cells=None, work=None):
    """The device form on the default stream.  Returns (cells [n_a, n_b + pad], self_a, self_b) as the host form does."""
    import torch

    a, b = _packed(case)
    da = _Dev(torch, a)
    db = da if b is None else _Dev(torch, b)
    ld = db.n + pad
    if cells is None:
        cells = torch.full((max(da.n, 1), max(ld, 1), 4), SENTINEL, dtype=torch.int64, device="cuda")
    need = compare.work_bytes(da.n, db.n, da.total, db.total)
    assert need > 0
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert work.numel() >= need
    compare.compare_device(*da.ptrs(), da.n, da.total, *db.ptrs(), db.n, db.total, case["keep_and"], case["keep_eq"],
                           cells.data_ptr(), ld, da.selfs.data_ptr(), db.selfs.data_ptr(), work.data_ptr(), work.numel(), 0)
    torch.cuda.synchronize()
    got = cells.cpu().numpy().view(np.uint64)[:da.n, :ld].copy().view(compare.CELL_DTYPE).reshape(da.n, ld)
    selfs = [d.selfs.cpu().numpy().view(np.uint64)[:d.n].copy().view(compare.SELF_DTYPE).reshape(d.n) for d in (da, db)]
    return got, selfs[0], selfs[1]


def _assert_equal(got, want, what):
    for g, w, part in zip(got, want, ("cells", "self_a", "self_b")):
        assert g.shape == w.shape, (what, part, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:5]
            raise AssertionError((what, part, [(tuple(ix), g[tuple(ix)], w[tuple(ix)]) for ix in bad]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_oracle_in_both_forms(hip_lib, name):
    case, want = CASES[name], expected(name)
    _assert_equal(_device(case), want, (name, "device form", windows_of(case)))
    _assert_equal(_host(case), want, (name, "host form", windows_of(case)))


SYMMETRIC = sorted(n for n, c in CASES.items() if c["b"] is None)


@pytest.mark.parametrize("name", SYMMETRIC)
def test_symmetric_call_equals_the_rectangular_call_and_its_transpose(hip_lib, name):
    case = CASES[name]
    rect = dict(case, b=[x.copy() for x in case["a"]], b_ab=case["a_ab"], b_keep=case["a_keep"])
    for form in (_device, _host):
        sym, s_a, s_b = form(case)
        full, r_a, r_b = form(rect)
        assert np.array_equal(sym, full) and np.array_equal(sym, sym.T), (name, form.__name__)
        assert np.array_equal(s_a, r_a) and np.array_equal(s_a, s_b) and np.array_equal(r_a, r_b)
        i = np.arange(s_a.size)  # cell (i, i) agrees with self row i
        for c_f, s_f in (("n_shared", "n_kept"), ("sum_min", "sum"), ("dot_lo", "sq_lo"), ("dot_hi", "sq_hi")):
            assert np.array_equal(sym[c_f][i, i], s_a[s_f]), (name, c_f)


@pytest.mark.parametrize("name", [f"tile_rect_{T + 1}x{T - 1}", "tile_sym_1", f"tile_sym_{2 * T + 1}", "windows_4_rect", "windows_4_sym", "all_empty"])
def test_nothing_is_written_outside_the_matrix(hip_lib, name):
    case, want = CASES[name], expected(name)
    n_b = want[2].size
    got = _device(case, pad=3)[0]
    _assert_equal((got[:, :n_b],), (want[0],), (name, "device"))
    assert (got[:, n_b:].view(np.uint64) == SENTINEL).all(), name
    buf = np.full((want[1].size, n_b + 3, 4), SENTINEL, dtype=np.uint64).view(compare.CELL_DTYPE).reshape(want[1].size, n_b + 3)
    got = _host(case, ld_cells=n_b + 3, cells=buf)[0]
    _assert_equal((got[:, :n_b],), (want[0],), (name, "host"))
    assert (got[:, n_b:].view(np.uint64) == SENTINEL).all(), name


def test_a_large_call_followed_by_a_small_one_leaves_nothing_stale(hip_lib):
    """The same cell, self-row and work buffers for a call of four windows and then for small ones of one window."""
    import torch

    big = CASES["windows_4_rect"]
    cells = torch.full((2 * T + 1, 2 * T + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")
    work = torch.full((compare.work_bytes(2, 2, 6000, 6000) + (1 << 16),), 0xFF, dtype=torch.uint8, device="cuda")
    assert windows_of(big) == 4
    _assert_equal(_device(big, cells=cells.view(-1)[:2 * 2 * 4].view(2, 2, 4), work=work), expected("windows_4_rect"), "large")
    for name in ("keep_nothing", "tile_rect_1x1", f"tile_sym_{T + 1}", "all_empty"):
        want = expected(name)
        n_a, n_b = want[1].size, want[2].size
        view = cells.view(-1)[:n_a * n_b * 4].view(n_a, n_b, 4)
        _assert_equal(_device(CASES[name], cells=view, work=work), want, ("small after large", name))


@pytest.mark.parametrize("name", ["panel_sym", "windows_8", "abund_max_on_three", "keep_known"])
def test_two_identical_calls_give_identical_bytes(hip_lib, name):
    for form in (_device, _host):
        first, second = form(CASES[name]), form(CASES[name])
        for x, y in zip(first, second):
            assert x.tobytes() == y.tobytes(), (name, form.__name__)


def test_n_shared_equals_the_overlap_of_the_batched_run_step(hip_lib):
    """Code that predates this pass: a database built from B, A run against it in one batch."""
    case = CASES["abund_both"]
    assert all(x.size for x in case["b"])
    with RefDB.from_sketches(case["b"]) as db:
        overlap = np.asarray(db.run_batch(case["a"])[0])
    got = _host(case)[0]
    assert overlap.shape == got.shape and np.array_equal(overlap.astype(np.uint64), got["n_shared"]) and got["n_shared"].sum() > 100
