"""The segmented sketch (yh_sketch_segments, yh_sketch_segments_device in yacht_amd/csrc/yh_sketch.hip) against
oracle/sketch_oracle.py, case by case (tests/sketch_seg_cases.py builds them and says what each is for;
tests/test_sketch_seg_cases_cpu.py checks their expectations without a GPU).  Every comparison is exact: array_equal on
mins, abund and off."""
import ctypes as C

import numpy as np
import pytest

import sketch_seg_cases as sg
from oracle import sketch_oracle as so

pytestmark = pytest.mark.gpu

# the geometry of yh_sketch.hip, by its names there
UNIT = 16              # bases per staged unit (one 16-byte load, one lcode/lbad word)
RL_RUN = 32            # windows per lane of the 2-bit kernels
RL_WIN = 8192          # windows per workgroup of the 2-bit kernels (RL_THREADS * RL_RUN)
SK_WIN = 2048          # windows per workgroup of the byte-wise kernel (SK_THREADS * SK_ITEMS)
SK_LCAP = 2048         # kept hashes a workgroup parks in LDS before they overflow to global memory
assert (UNIT, RL_RUN, RL_WIN, SK_WIN, SK_LCAP) == (sg.UNIT, sg.RL_RUN, sg.RL_WIN, sg.SK_WIN, sg.SK_LCAP)

PREFILL = 0xA5A5A5A5A5A5A5A5
PREFILL32 = 0xA5A5A5A5
CANARY = 64


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


def host_form(lib, buf, seg_off, k, scaled, cap_mins, seed=42, n_bytes=None):
    """yh_sketch_segments -> (rc, n_out, mins[cap], abund[cap], off, the canary words behind mins and abund)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
    n_seg = seg_off.size - 1
    mins = np.full(cap_mins + CANARY, PREFILL, dtype=np.uint64)
    abund = np.full(cap_mins + CANARY, PREFILL32, dtype=np.uint32)
    off = np.full(n_seg + 1 + CANARY, PREFILL, dtype=np.uint64)
    n_out = C.c_uint64(12345)
    rc = lib.yh_sketch_segments(_vp(buf), buf.size if n_bytes is None else n_bytes, _vp(seg_off), n_seg, k, seed,
                                so.max_hash_for_scaled(scaled), 0, cap_mins, _vp(mins) if cap_mins else None,
                                _vp(abund) if cap_mins else None, _vp(off), C.byref(n_out))
    assert bool(np.all(off[n_seg + 1:] == np.uint64(PREFILL)))
    return rc, int(n_out.value), mins[:cap_mins], abund[:cap_mins], off[:n_seg + 1], (mins[cap_mins:], abund[cap_mins:])


def device_form(lib, buf, seg_off, k, scaled, cap_kept, cap_mins, shift=0, seed=42):
    """yh_sketch_segments_device on the buffer placed `shift` bytes into a 16-byte aligned device buffer, padded with 'A'
    (valid bases: a read outside a segment shows as extra hashes) -> (rc, totals, mins[cap], abund[cap], off); asserts that
    the words behind cap_mins, behind off and behind the work buffer are as they were"""
    import torch

    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
    n, n_seg = int(buf.size), seg_off.size - 1
    d_buf = torch.full((shift + n + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert d_buf.data_ptr() % 16 == 0
    if n:
        d_buf[shift:shift + n] = torch.from_numpy(np.array(buf))
    d_seq = d_buf[shift:]
    d_segoff = torch.from_numpy(seg_off.view(np.int64).copy()).cuda()
    wb = int(lib.yh_sketch_segments_work_bytes(cap_kept, n_seg))
    assert wb > 0, lib.yh_last_error()
    work = torch.full((wb + CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
    mins = torch.full((cap_mins + CANARY,), PREFILL - 2 ** 64, dtype=torch.int64, device="cuda")
    abund = torch.full((cap_mins + CANARY,), PREFILL32 - 2 ** 32, dtype=torch.int32, device="cuda")
    off = torch.full((n_seg + 1 + CANARY,), PREFILL - 2 ** 64, dtype=torch.int64, device="cuda")
    totals = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rc = lib.yh_sketch_segments_device(C.c_void_p(d_seq.data_ptr()) if n else None, n, C.c_void_p(d_segoff.data_ptr()), n_seg, k, seed,
                                       so.max_hash_for_scaled(scaled), cap_kept, C.c_void_p(work.data_ptr()), wb, cap_mins,
                                       C.c_void_p(mins.data_ptr()), C.c_void_p(abund.data_ptr()), C.c_void_p(off.data_ptr()),
                                       C.c_void_p(totals.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    mins_h = mins.cpu().numpy().view(np.uint64)
    abund_h = abund.cpu().numpy().view(np.uint32)
    off_h = off.cpu().numpy().view(np.uint64)
    assert bool(np.all(mins_h[cap_mins:] == np.uint64(PREFILL))) and bool(np.all(abund_h[cap_mins:] == np.uint32(PREFILL32)))
    assert bool(np.all(off_h[n_seg + 1:] == np.uint64(PREFILL))) and bool(np.all(work[wb:].cpu().numpy() == 0x5A))
    return rc, [int(x) for x in totals.cpu().numpy()], mins_h[:cap_mins], abund_h[:cap_mins], off_h[:n_seg + 1]


def _check_case(lib, case):
    from yacht_amd import _lib

    name, k, scaled = case["name"], case["k"], case["scaled"]
    want_m, want_a, want_o = sg.expected(name)
    T, D = sg.kept_total(name), want_m.size
    n_win = max(case["buf"].size - k + 1, 0)
    # the device form, with room for every window and then with exactly the room it needs
    for cap_kept, cap_mins in ((n_win, n_win), (T, D)):
        rc, totals, m, a, o = device_form(lib, case["buf"], case["seg_off"], k, scaled, cap_kept, cap_mins, shift=case["shift"])
        assert rc == _lib.YH_OK, (name, lib.yh_last_error())
        assert totals == [T, D], (name, totals, T, D)
        assert np.array_equal(o, want_o), name
        assert np.array_equal(m[:D], want_m) and np.array_equal(a[:D], want_a), name
        assert bool(np.all(m[D:] == np.uint64(PREFILL))) and bool(np.all(a[D:] == np.uint32(PREFILL32))), name
    # the host form (its own aligned buffer: a shifted case runs the 2-bit kernel here, with the same answer)
    rc, n_out, m, a, o, canary = host_form(lib, case["buf"], case["seg_off"], k, scaled, D)
    assert rc == _lib.YH_OK and n_out == D, (name, rc, n_out, lib.yh_last_error())
    assert np.array_equal(o, want_o) and np.array_equal(m, want_m) and np.array_equal(a, want_a), name
    assert bool(np.all(canary[0] == np.uint64(PREFILL))) and bool(np.all(canary[1] == np.uint32(PREFILL32))), name


# ---- 1 .. 5 and the small ones: every case through both forms ---------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in sg.all_cases()])
def test_case_equals_the_oracle(hip_lib, name):
    _check_case(hip_lib, sg.case_named(name))


def test_python_entry_and_same_bytes_twice(hip_lib):
    from yacht_amd import sketch

    for name in ("tiny-k21", "real-s100", "lowcomplex-s2"):
        case = sg.case_named(name)
        want = sg.expected(name)
        got = sketch.sketch_segments(case["buf"], case["seg_off"], case["k"], case["scaled"])
        assert [g.dtype for g in got] == [np.uint64, np.uint32, np.uint64]
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
    case = sg.case_named("overflow-s2")
    n_win = case["buf"].size - case["k"] + 1
    runs = [device_form(hip_lib, case["buf"], case["seg_off"], case["k"], case["scaled"], n_win, n_win) for _ in range(2)]
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][2:], runs[1][2:])) and runs[0][1] == runs[1][1]


# ---- 6: capacity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["overflow-s4", "strands-k31"])
def test_capacity(hip_lib, name):
    from yacht_amd import _lib

    case = sg.case_named(name)
    k, scaled = case["k"], case["scaled"]
    want_m, want_a, want_o = sg.expected(case["name"])
    T, D = sg.kept_total(case["name"]), want_m.size
    assert T >= D > SK_LCAP and (name != "strands-k31" or T == 2 * D)
    # device form, one pair short: the count says so, nothing behind the caps is touched (device_form asserts the canaries)
    rc, totals, m, a, o = device_form(hip_lib, case["buf"], case["seg_off"], k, scaled, T - 1, D)
    assert rc == _lib.YH_OK and totals[0] == T and totals[1] <= D
    assert o[0] == 0 and int(o[-1]) == totals[1] and bool(np.all(o[1:] >= o[:-1]))
    # ... one sketch entry short: both totals exact, off complete, the entries that fit are the first ones
    rc, totals, m, a, o = device_form(hip_lib, case["buf"], case["seg_off"], k, scaled, T, D - 1)
    assert rc == _lib.YH_OK and totals == [T, D] and np.array_equal(o, want_o)
    assert np.array_equal(m, want_m[:D - 1]) and np.array_equal(a, want_a[:D - 1])
    # ... and a retry with the reported sizes
    rc, totals, m, a, o = device_form(hip_lib, case["buf"], case["seg_off"], k, scaled, totals[0], totals[1])
    assert rc == _lib.YH_OK and totals == [T, D]
    assert np.array_equal(o, want_o) and np.array_equal(m, want_m) and np.array_equal(a, want_a)
    # cap_mins = 0: counts and offsets only
    rc, totals, m, a, o = device_form(hip_lib, case["buf"], case["seg_off"], k, scaled, T, 0)
    assert rc == _lib.YH_OK and totals == [T, D] and np.array_equal(o, want_o)
    # host form
    rc, n_out, m, a, o, canary = host_form(hip_lib, case["buf"], case["seg_off"], k, scaled, D - 1)
    assert rc == _lib.YH_ERR_CAPACITY and n_out == D and np.array_equal(o, want_o)
    assert bool(np.all(canary[0] == np.uint64(PREFILL))) and bool(np.all(canary[1] == np.uint32(PREFILL32)))
    rc, n_out, m, a, o, canary = host_form(hip_lib, case["buf"], case["seg_off"], k, scaled, 0)
    assert rc == _lib.YH_OK and n_out == D and np.array_equal(o, want_o)
    rc, n_out, m, a, o, canary = host_form(hip_lib, case["buf"], case["seg_off"], k, scaled, n_out)
    assert rc == _lib.YH_OK and n_out == D
    assert np.array_equal(o, want_o) and np.array_equal(m, want_m) and np.array_equal(a, want_a)


# ---- 7: arguments (host form) ------------------------------------------------------------------------------------------------
def test_arguments(hip_lib):
    from yacht_amd import _lib

    buf = np.array(sg.case_named("small-k21")["buf"])
    n = buf.size
    for what, off, n_bytes in (("descending", [0, 50, 40, n], None), ("first", [1, 50, n], None), ("last short", [0, 50, n - 1], None),
                               ("last long", [0, 50, n + 1], None), ("4 GiB", [0, 50, 2 ** 32], 2 ** 32),
                               ("above", [0, 50, 2 ** 32 + 5], 2 ** 32 + 5)):
        rc, n_out, m, a, o, canary = host_form(hip_lib, buf, off, 21, 1, 64, n_bytes=n_bytes)
        assert rc == _lib.YH_ERR_INVALID_ARG and n_out == 0, what
        assert bool(np.all(m == np.uint64(PREFILL))) and bool(np.all(a == np.uint32(PREFILL32))), what
    for ksize in (0, 256):
        assert host_form(hip_lib, buf, [0, n], ksize, 1, 64)[0] == _lib.YH_ERR_INVALID_ARG
    # no segment: an empty result, off = [0]
    rc, n_out, m, a, o, canary = host_form(hip_lib, np.zeros(0, np.uint8), [0], 21, 1, 64)
    assert rc == _lib.YH_OK and n_out == 0 and o.tolist() == [0]
    rc, totals, m, a, o = device_form(hip_lib, np.zeros(0, np.uint8), [0], 21, 1, 16, 16)
    assert rc == _lib.YH_OK and totals == [0, 0] and o.tolist() == [0]
    # segments but nothing as long as k
    rc, n_out, m, a, o, canary = host_form(hip_lib, buf[:10], [0, 4, 10], 21, 1, 64)
    assert rc == _lib.YH_OK and n_out == 0 and o.tolist() == [0, 0, 0]
    rc, totals, m, a, o = device_form(hip_lib, buf[:10], [0, 4, 10], 21, 1, 16, 16)
    assert rc == _lib.YH_OK and totals == [0, 0] and o.tolist() == [0, 0, 0]


# ---- 8: one segment = the unsegmented call, sorted and counted ---------------------------------------------------------------
@pytest.mark.parametrize("k,scaled", [(31, 1), (51, 7), (70, 3)])
def test_one_segment_equals_the_unsegmented_call(hip_lib, k, scaled):
    from yacht_amd import sketch

    buf = np.array(sg.case_named("overflow-s2")["buf"])
    m1, c1 = np.unique(sketch.hash_kmers([buf], k, scaled), return_counts=True)
    mins, abund, off = sketch.sketch_segments(buf, [0, buf.size], k, scaled)
    assert off.tolist() == [0, m1.size] and np.array_equal(mins, m1) and np.array_equal(abund, c1.astype(np.uint32))
    # (the oracle stays the reference)
    h = so.kmer_hashes(buf.tobytes(), k)
    m0, c0 = np.unique(h[h <= np.uint64(so.max_hash_for_scaled(scaled))], return_counts=True)
    assert np.array_equal(mins, m0) and np.array_equal(abund, c0.astype(np.uint32))
