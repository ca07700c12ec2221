"""The database build refuses a sketch that is not strictly ascending on EVERY path that sorts it.

The ordering check rides along with whichever pass reads the pairs anyway ("Where the sketch order is checked"), so
each row below pins one path, in three steps:
  1. the clean base builds, takes the path the row is named for (info()["sort_path"], the verdict lines of YH_TRACE_BUILD) and
     answers as the oracle does -- a row whose clean build takes another path FAILS, it does not pass vacuously;
  2. every bad case of the base (tests/order_cases.py: one violation at a wave, load-round, item, tile, sketch or chunk edge)
     is refused, as host arrays and -- unchunked rows -- as device arrays: YH_ERR_UNSORTED with "not strictly ascending" in
     yh_last_error(), YH_ERR_INVALID_ARG for offsets[0] = 1; refusals counted == cases generated, both printed;
  3. the clean base is built again in the same process and answers exactly as in step 1 (a refused create leaves nothing
     behind in the buffer cache, the flag words or the pinned rows).
Tuning variables are read when the library is first used: one child process per row, one after another.

The `above_max` case (an interior element 2^64 - 2 above the largest LAST element, so the largest hash the extents pass reports
is exceeded by the data) runs on every row.  What was read to allow that -- every index derived from a key is clamped or
masked before it is used, or its kernel runs only behind the verdict:
  k_part            bin_of: `x >= a.nbins ? a.nbins - 1 : x`; the bin is the region index, stores guarded by `at < a.cap_out`
  k_piece_bounds    `reg = reg >= a.P1 ? a.P1 - 1u : reg` (rows of W = P1 + 1 words)
  k_piece_part      the same clamp, `if (reg != r) { bad = true; b = 0; }`, `if (b >= a.P2) b = a.P2 - 1u`, stores guarded by
                    `at < BKT_CAP`; positions come from the bounds, not from keys
  k_bucket_sort     `slot = fine_of(...) & (BKT_SLOTS - 1u)`; output at off[b] + i with i < the bucket's count
  k_bucket_group    `s = fine_of(...) & (BKT_CAP - 1u)`, probes `& (BKT_CAP - 1u)`; key + 1 != 0 for 2^64 - 2
  k_bucket_group5   `s = (u32)(mixed >> (64 - BKT_SLOT_BITS))`, steps `& (BKT_CAP - 1u)`; records only at `val[k] < a.n_pos`
  k_spill_collect / k_spill_place   index a bit map / the bucket offsets by bucket_of(h): they run only when no flag bit is
                    set ((hflags[0] & 15u) == 0, and the misplaced key sets bit 8), and clamp the bucket to the last one
  k_scan_refs / yh_build_check_order   compare keys, index nothing by them; the radix sort runs behind the verdict
  chunked upload    validate_end reads k_scan_refs' verdict before k_piece_part / the second level run

Offsets that overshoot the values array are tested through the device form only, with an allocation larger than the largest
bogus offset: no read can leave the allocation whatever the guard in k_ref_extents does.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import json, os, sys
import numpy as np
root, base_name, flags_list, forms = sys.argv[1], sys.argv[2], [int(x) for x in sys.argv[3].split(",")], sys.argv[4].split(",")
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch
import order_cases as oc
from oracle import oracle
from yacht_amd import _lib
from yacht_amd.engine import RefDB, YH_DB_NO_INDEX, YH_DB_PAIRWISE_ONLY

def say(msg):
    sys.stderr.flush()
    print("[order] " + msg, file=sys.stderr, flush=True)

b = oc.base(base_name)
values, offsets = np.array(b.values), np.array(b.offsets)
cases = oc.all_cases(base_name)
rng = np.random.default_rng(7)
picks = [b.targets["start0"], b.targets["cross1024"], 0, b.n_refs // 2]
sample = np.unique(np.concatenate([b.sketch(j)[::3] for j in picks] + [values[rng.integers(0, b.H, 300)],
                                  rng.integers(1, max(b.max_hash, 2), size=500, dtype=np.uint64)]))
want_ov = oracle.overlap(values, offsets, sample, threads=4)
want_e, want_m = oracle.exclusive(values, offsets, want_ov > 0, sample)
wi, wj, wc, wstats = oracle.train_pairs(values, offsets, 0.0, threads=4)

def answers(db, flags):
    # (what the handle answers, is it the oracle's answer)
    if flags & YH_DB_PAIRWISE_ONLY:
        gi, gj, gc = db.pairwise(0.0)
        got = [gi, gj, gc, np.array(db.index_stats(), np.uint64)]
        ok = np.array_equal(gi, wi) and np.array_equal(gj, wj) and np.array_equal(gc, wc) and db.index_stats() == wstats
    elif flags & YH_DB_NO_INDEX:
        got = [db.overlap(sample)]
        ok = np.array_equal(got[0], want_ov)
    else:
        ov, e, m = db.run_counts(sample)
        got = [ov, e, m]
        ok = np.array_equal(ov, want_ov) and np.array_equal(e, want_e) and np.array_equal(m, want_m)
    return got, bool(ok)

def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")

def create(v, o, flags, form):
    if form == "host":
        return RefDB(v, o, flags=flags)
    dv, do = to_device(v), to_device(o)
    torch.cuda.synchronize()
    return RefDB.from_device(dv.data_ptr(), do.data_ptr(), o.size - 1, flags=flags)

out = {"base": base_name, "n_cases": len(cases), "H": b.H, "n_refs": b.n_refs, "pairs": int(wi.size), "overlapping": int((want_ov > 0).sum()), "rows": {}}
for flags in flags_list:
    row = {"wrong": [], "refused": 0}
    say(f"clean-begin flags={flags}")
    with create(values, offsets, flags, forms[0]) as db:
        first, row["clean_ok"] = answers(db, flags)
        row["sort_path"] = int(db.info()["sort_path"])
    say(f"clean-end flags={flags}")
    for name, _, _, bv, bo, site in cases:
        want = _lib.YH_ERR_INVALID_ARG if oc.expected_error(name) == "invalid_arg" else _lib.YH_ERR_UNSORTED
        for form in forms:
            try:
                db = create(bv, bo, flags, form)
            except _lib.YachtHipError as ex:
                if ex.code == want and (want != _lib.YH_ERR_UNSORTED or "not strictly ascending" in str(ex)):
                    row["refused"] += 1
                else:
                    row["wrong"].append([name, form, f"code {ex.code}: {ex}"])
            else:
                db.close()
                row["wrong"].append([name, form, "BUILT"])
    say(f"again-begin flags={flags}")
    with create(values, offsets, flags, forms[0]) as db:
        again, again_ok = answers(db, flags)
        row["again_sort_path"] = int(db.info()["sort_path"])
    say(f"again-end flags={flags}")
    row["again_ok"] = bool(again_ok and len(again) == len(first) and all(np.array_equal(x, y) for x, y in zip(first, again)))
    out["rows"][str(flags)] = row
print(json.dumps(out))
"""

PAIRWISE_ONLY, NO_INDEX = 8, 1
FORCED_TWO_LEVEL = {"YH_NO_PIECES": "1", "YH_NO_PIECES_SORT": "1"}
CHUNKED = {"YH_UPLOAD_CHUNK_MIN": "1", "YH_UPLOAD_SHARES": "0.4,0.3,0.2,0.1"}

# row -> (base, flags of its handles, environment, forms, {flags: (sort_path, which verdict line the clean build must print)})
# verdict: (prefix of the line, text it contains, how it ends) or None: no distribution sort may report at all
ROWS = {
    "train_pieces": ("A", [PAIRWISE_ONLY], {}, "host,device", {PAIRWISE_ONLY: (3, ("[yh pieces]", "records of", "taken"))}),
    "train_two_level": ("B", [PAIRWISE_ONLY], {}, "host,device", {PAIRWISE_ONLY: (2, ("[yh sort]", "fused: records of", "taken"))}),
    "train_two_level_forced_tile_edges": ("A", [PAIRWISE_ONLY], {"YH_NO_PIECES": "1"}, "host,device",
                                          {PAIRWISE_ONLY: (2, ("[yh sort]", "fused: records of", "taken"))}),
    "full_pieces": ("A", [0], {}, "host,device", {0: (3, ("[yh pieces]", " sorted ", "taken"))}),
    "full_two_level_forced": ("A", [0], FORCED_TWO_LEVEL, "host,device", {0: (2, ("[yh sort]", " sorted ", "taken"))}),
    "two_level_natural_full_range": ("C", [0, PAIRWISE_ONLY], {}, "host,device",
                                     {0: (2, ("[yh sort]", " sorted ", "taken")), PAIRWISE_ONLY: (2, ("[yh sort]", " sorted ", "taken"))}),
    "own_pass": ("D", [0], {}, "host,device", {0: (1, None)}),
    "refused_keys": ("R", [0], FORCED_TWO_LEVEL, "host,device", {0: (1, ("[yh sort]", " sorted ", "REFUSED"))}),
    "chunked_upload": ("A", [0, PAIRWISE_ONLY], CHUNKED, "host",
                       {0: (2, ("[yh sort]", " sorted ", "taken")), PAIRWISE_ONLY: (3, ("[yh pieces]", "records of", "taken"))}),
    "no_index": ("A", [NO_INDEX], {}, "host,device", {NO_INDEX: (3, ("[yh pieces]", " sorted ", "taken"))}),
}


def _segment(lines, flags, which):
    a = lines.index(f"[order] {which}-begin flags={flags}")
    z = lines.index(f"[order] {which}-end flags={flags}")
    return lines[a + 1:z]


@pytest.mark.parametrize("row", list(ROWS))
def test_every_sort_path_refuses_every_violation(hip_lib, row):
    base, flags_list, env_extra, forms, expect = ROWS[row]
    env = dict(os.environ)
    env.update({"YH_DEBUG_TUNING": "1", "YH_TRACE_BUILD": "1"})
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", WORKER, ROOT, base, ",".join(str(f) for f in flags_list), forms],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    lines = [ln.rstrip() for ln in r.stderr.splitlines()]
    n_forms = len(forms.split(","))
    assert out["n_cases"] > 80 and out["H"] < 10 ** 4
    assert out["pairs"] > 0 and out["overlapping"] > 3          # (the oracle comparison compares something)
    for flags in flags_list:
        got = out["rows"][str(flags)]
        print(f"{row} flags {flags}: {out['n_cases']} cases x {n_forms} forms generated, {got['refused']} refusals, "
              f"{len(got['wrong'])} wrong, sort_path {got['sort_path']}")
        want_path, verdict = expect[flags]
        # 1. the clean build: this row's path, the oracle's answers
        for which in ("clean", "again"):
            seg = _segment(lines, flags, which)
            verdicts = [ln for ln in seg if (ln.startswith("[yh sort]") or ln.startswith("[yh pieces]")) and " -> " in ln]
            if verdict is None:
                assert not verdicts, verdicts
            else:
                prefix, text, end = verdict
                assert len(verdicts) == 1 and verdicts[0].startswith(prefix) and text in verdicts[0] and verdicts[0].endswith("-> " + end), (which, verdicts)
            if row == "chunked_upload":   # (the database went up in the four chunks the targets are laid around)
                assert sum("chunk work queued" in ln for ln in seg) == 4, seg
            else:
                assert not any("chunk work queued" in ln for ln in seg)
        assert got["sort_path"] == want_path == got["again_sort_path"], got
        assert got["clean_ok"], (row, flags, "the clean build does not answer as the oracle")
        # 2. every bad case refused, with its own code and message, in every form
        assert got["wrong"] == [], got["wrong"][:12]
        assert got["refused"] == out["n_cases"] * n_forms
        # 3. the same answers behind all the refusals
        assert got["again_ok"], (row, flags, "the rebuilt clean base answers differently")


@pytest.mark.parametrize("flags", [0, PAIRWISE_ONLY])
def test_offsets_beyond_the_values_are_refused(hip_lib, flags):
    """offsets = [0, 3000, 100, 100] over H = 100 hashes: the second offset overshoots the database.  k_ref_extents flags an
    offset above offsets[n_refs] like one below its predecessor and reads nothing through it.  The values tensor here has 4 096
    elements, more than the largest offset, so this test cannot read outside its allocation with or without that guard."""
    import torch

    from yacht_amd import _lib
    from yacht_amd.engine import RefDB

    vals = np.arange(1, 4097, dtype=np.int64) * 1000003
    for offs in ([0, 3000, 100, 100], [0, 100, 3000, 100], [0, 4096, 4096, 100]):
        assert max(offs) <= vals.size and offs[-1] == 100
        dv = torch.from_numpy(vals).to("cuda:0")
        do = torch.tensor(offs, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(_lib.YachtHipError) as ei:
            RefDB.from_device(dv.data_ptr(), do.data_ptr(), len(offs) - 1, flags=flags)
        assert ei.value.code == _lib.YH_ERR_UNSORTED, offs
        assert "not strictly ascending" in str(ei.value)
    # the same arrays with honest offsets build: the refusal was about the offsets
    do = torch.tensor([0, 30, 100, 100], dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with RefDB.from_device(dv.data_ptr(), do.data_ptr(), 3, flags=flags) as db:
        assert db.info()["n_hashes"] == 100
