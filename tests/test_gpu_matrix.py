"""yh_matrix_cells_device, yh_matrix_prevalence_device and yh_matrix_fill_device on the GPU against the loop oracle of
tests/matrix_cases.py, at the smallest shapes where they can go wrong: databases of 5 and 300 references, row counts around
the compaction chunk, runs over a wave and a workgroup's tile, sums over 2^32 and 2^40, outputs pre-filled with 0xFF."""
import matrix_cases as mc
import numpy as np
import pytest

from yacht_amd import _lib, abundance
from yacht_amd.engine import MATRIX_CELL_DTYPE, RefDB

pytestmark = pytest.mark.gpu

CELLS = mc.cells_cases()
PREV = mc.prevalence_cases()
FILL = mc.fill_cases()


def _ids(cases):
    return [c["name"] for c in cases]


@pytest.fixture(scope="module")
def dbs(hip_lib):
    """One resident database per N: the passes read nothing of it but N."""
    made = {n: RefDB.from_sketches([np.arange(1 + 10 * j, 6 + 10 * j, dtype=np.uint64) for j in range(n)]) for n in (5, 300)}
    yield made
    for db in made.values():
        db.close()


def _dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cells_call(db, case, torch, n_sets=None, fill_byte=0xFF):
    rows, present, med = case["rows"], case["present"], case["med"]
    cap = len(rows)
    d_rows = _dev(rows.view(np.int32), torch)
    d_n = torch.tensor([case["n_rows"]], dtype=torch.int32).cuda()
    d_present = _dev(present, torch)
    d_med = _dev(med, torch) if med is not None else None
    d_cells = torch.full((cap, 3), -1 if fill_byte else 0, dtype=torch.int64).cuda()
    d_count = torch.full((1,), -1, dtype=torch.int64).cuda()
    db.matrix_cells_device(d_rows.data_ptr(), d_n.data_ptr(), cap, d_present.data_ptr(), len(present) if n_sets is None else n_sets,
                           d_med.data_ptr() if d_med is not None else 0, case["base"], d_cells.data_ptr(), d_count.data_ptr())
    db.synchronize()
    torch.cuda.synchronize()
    n = int(d_count.item())
    assert 0 <= n <= cap
    got = d_cells.cpu().numpy()
    assert (got[n:] == -1).all()  # nothing written behind the count
    return got[:n].reshape(-1).view(MATRIX_CELL_DTYPE)


@pytest.mark.parametrize("case", CELLS, ids=_ids(CELLS))
def test_cells(dbs, case):
    import torch

    db = dbs[case["n_refs"]]
    want = mc.cells_oracle(case["rows"], case["n_rows"], case["present"], case["med"], case["base"], case["n_refs"])
    got = _cells_call(db, case, torch)
    assert got.size == want.size and got.tobytes() == want.tobytes()
    again = _cells_call(db, case, torch)
    assert again.tobytes() == got.tobytes()  # two identical calls: identical bytes
    if case["name"] == "large_medians":
        assert int(got["depth2"].max()) == 2 ** 33 - 1 and int(got["depth2"].min()) == 1


def test_cells_argument_checks(dbs):
    import torch

    case = CELLS[2]
    for n_sets in (0, 33):
        with pytest.raises(_lib.YachtHipError) as ei:
            _cells_call(dbs[5], case, torch, n_sets=n_sets)
        assert ei.value.code == _lib.YH_ERR_INVALID_ARG
    for call in (lambda: dbs[5].matrix_prevalence_device(0, 0, 0, 1, 0, 0, 0), lambda: dbs[5].matrix_prevalence_device(0, 0, 33, 1, 0, 0, 0)):
        with pytest.raises(_lib.YachtHipError) as ei:
            call()
        assert ei.value.code == _lib.YH_ERR_INVALID_ARG


def _prevalence_call(db, case, torch):
    cells, n_sets, S, N = case["cells"], case["n_sets"], case["n_samples"], case["n_refs"]
    d_cells = _dev(cells.view(np.int64).reshape(-1, 3), torch) if cells.size else torch.zeros((1, 3), dtype=torch.int64).cuda()
    d_skip = _dev(case["skip"], torch) if case["skip"] is not None else None
    d_prev = torch.full((n_sets, N), -1, dtype=torch.int32).cuda()  # (0xFF everywhere)
    d_denom = torch.full((n_sets, S), -1, dtype=torch.int64).cuda()
    db.matrix_prevalence_device(d_cells.data_ptr(), cells.size, n_sets, S, d_skip.data_ptr() if d_skip is not None else 0,
                                d_prev.data_ptr(), d_denom.data_ptr())
    db.synchronize()
    torch.cuda.synchronize()
    return d_prev.cpu().numpy().view(np.uint32), d_denom.cpu().numpy().view(np.uint64), d_cells, d_skip, d_denom


@pytest.mark.parametrize("case", PREV, ids=_ids(PREV))
def test_prevalence(dbs, case):
    import torch

    want_p, want_d = mc.prevalence_oracle(case["cells"], case["n_sets"], case["n_samples"], case["skip"], case["n_refs"])
    got_p, got_d = _prevalence_call(dbs[case["n_refs"]], case, torch)[:2]
    assert np.array_equal(got_p, want_p) and np.array_equal(got_d, want_d)
    if case["name"] == "sums_over_2^32_and_2^40":
        assert int(got_d[0, 0]) > 1 << 40 and 1 << 32 < int(got_d[0, 1]) < 1 << 40
    if case["name"] in ("no_cells", "skip_all"):
        assert not got_p.any() and not got_d.any()


@pytest.mark.parametrize("case", FILL, ids=_ids(FILL))
def test_fill(dbs, case):
    import torch

    db = dbs[case["n_refs"]]
    S, bit = case["n_samples"], case["bit"]
    _p, denom, d_cells, d_skip, d_denom = _prevalence_call(db, case, torch)
    row_of, n_kept = mc.row_of_ref(case["kept"]), int(case["kept"].sum())
    want = mc.fill_oracle(case["cells"], bit, S, case["skip"], row_of, n_kept, denom[bit], case["want_rel"])
    d_row = _dev(row_of, torch)
    shape = (max(n_kept, 1), S)
    d_pres = torch.full(shape, -1, dtype=torch.int8).cuda()  # (0xFF everywhere)
    d_nm = torch.full(shape, -1, dtype=torch.int32).cuda()
    d_rel = torch.full(shape, -1, dtype=torch.int64).cuda() if case["want_rel"] else None
    db.matrix_fill_device(d_cells.data_ptr(), case["cells"].size, bit, S, d_skip.data_ptr() if d_skip is not None else 0, d_row.data_ptr(),
                          n_kept, d_denom[bit].data_ptr(), d_pres.data_ptr(), d_nm.data_ptr(), d_rel.data_ptr() if d_rel is not None else 0)
    db.synchronize()
    torch.cuda.synchronize()
    pres, nm = d_pres.cpu().numpy().view(np.uint8), d_nm.cpu().numpy().view(np.uint32)
    if n_kept == 0:  # nothing launched, nothing touched
        assert (pres == 0xFF).all() and (nm == 0xFFFFFFFF).all()
        return
    assert np.array_equal(pres, want[0]) and np.array_equal(nm, want[1])  # (fully defined: no 0xFF byte survives)
    if case["want_rel"]:
        rel = d_rel.cpu().numpy().view(np.uint64)
        assert np.array_equal(rel, want[2].view(np.uint64))
    if case["name"] == "bit_in_no_cell":
        assert not pres.any() and not nm.any()
    if case["name"] == "zero_denominator":
        assert int(denom[bit][4]) == 0 and pres[:, 4].any() and not d_rel.cpu().numpy()[:, 4].any()


def test_rel_equals_abundance_columns_bit_for_bit(dbs):
    """One sample over 300 references: the quotient of the fill equals abundance.abundance_columns' depth / total."""
    import torch

    rng = np.random.default_rng(11)
    N = 300
    med = rng.integers(1, 100000, N).astype(np.float64) / 2.0  # x.0 and x.5
    n_m = rng.integers(0, 50, N)
    present = (rng.random(N) < 0.6) & (n_m > 0)
    host = abundance.abundance_columns(np.ones(N), np.ones(N), med, np.ones(N), n_m, present, 1)["relative_abundance"].to_numpy()
    cells = np.zeros(int(present.sum()), dtype=MATRIX_CELL_DTYPE)
    cells["ref"], cells["n_match"], cells["mask"] = np.flatnonzero(present), n_m[present], 1
    cells["depth2"] = (2 * med[present]).astype(np.uint64)
    case = dict(cells=cells, n_sets=1, n_samples=1, n_refs=N, skip=None)
    _p, denom, d_cells, _s, d_denom = _prevalence_call(dbs[N], case, torch)
    assert int(denom[0, 0]) == int(2 * med[present].sum())
    d_row = _dev(np.arange(N, dtype=np.int32), torch)
    d_pres, d_nm = torch.zeros((N, 1), dtype=torch.uint8).cuda(), torch.zeros((N, 1), dtype=torch.int32).cuda()
    d_rel = torch.zeros((N, 1), dtype=torch.float64).cuda()
    dbs[N].matrix_fill_device(d_cells.data_ptr(), cells.size, 0, 1, 0, d_row.data_ptr(), N, d_denom[0].data_ptr(), d_pres.data_ptr(),
                              d_nm.data_ptr(), d_rel.data_ptr())
    dbs[N].synchronize()
    torch.cuda.synchronize()
    rel = d_rel.cpu().numpy()[:, 0]
    assert np.array_equal(rel.view(np.uint64), host.view(np.uint64)) and abs(rel.sum() - 1.0) <= 1e-12
