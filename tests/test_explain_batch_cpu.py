"""The batched explain without a GPU: the header declares the three entries (the ABI stays 8), the library exports them and
refuses a null handle and a bad block size, the binding types them, and RefDB.explain_batch checks the member rows on the
host before any library call."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from yacht_amd import _lib, cohort, engine

ENTRIES = ("yh_explain_members_rows_device", "yh_explain_batch_device", "yh_explain_batch")


def _header():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        return f.read()


def test_header_declares_the_entries_and_the_abi_stays_8():
    text = _header()
    for name in ENTRIES:
        assert f"int {name}(" in text, name
    assert "#define YH_ABI_VERSION 8" in text
    table = text[text.index("entry point   "):text.index("#define YH_RUN_CONTEXTS")]
    assert "yh_explain_batch / yh_explain_batch_device" in table and "yh_explain_members_rows_device" in table
    assert f"#define YH_EXPLAIN_BATCH_TILE {_lib.YH_EXPLAIN_BATCH_TILE}\n" in text


def test_binding_types_the_entries():
    assert [len(_lib.SIGNATURES[name][1]) for name in ENTRIES] == [8, 9, 8]
    for name in ("explain_members_rows_device", "explain_batch_device", "explain_batch"):
        assert callable(getattr(engine.RefDB, name))


def test_library_exports_the_entries_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.yh_abi_version() == 8
    for name in ENTRIES:
        assert hasattr(lib, name), name
    buf = np.zeros(64, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.yh_explain_members_rows_device(None, p, p, 4, p, 7, 1, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_explain_batch_device(None, p, p, None, 1, 0, p, None, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_explain_batch(None, p, p, None, 1, p, None, p) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()


def test_explain_batch_checks_the_member_rows_before_any_library_call():
    db = engine.RefDB.__new__(engine.RefDB)  # no handle: the checks come before any library call
    db._h = C.c_void_p(0)
    db.n_refs = 3
    samples = [np.arange(1, 6, dtype=np.uint64), np.zeros(0, np.uint64)]
    good = np.array([[0, 1, 127], [5, 0, 0]], np.uint8)
    assert engine.check_members(good.tolist(), 2, 3).dtype == np.uint8
    for bad in (good[0], good[:1], good[:, :2], np.zeros((2, 3, 1), np.uint8), good.T):
        with pytest.raises(ValueError, match=r"\[n_samples, n_refs\]"):
            db.explain_batch(samples, bad)
    for value in (0x80, 0xFF, 200):
        bad = good.astype(np.int64)
        bad[1, 2] = value
        with pytest.raises(ValueError, match="bit 7 must be clear"):
            db.explain_batch(samples, bad)
    with pytest.raises(ValueError, match="bit 7 must be clear"):
        db.explain_batch(samples, good.astype(np.int64) - 1)
    with pytest.raises(ValueError, match="integers"):
        db.explain_batch(samples, good.astype(np.float64))
    with pytest.raises(ValueError, match="1..256 samples"):
        db.explain_batch([], np.zeros((0, 3), np.uint8))
    with pytest.raises(ValueError, match="1..256 samples"):
        db.explain_batch([samples[0]] * 257, np.zeros((257, 3), np.uint8))
    with pytest.raises(ValueError, match="abundance arrays"):
        db.explain_batch(samples, good, abunds=[None])
    with pytest.raises(ValueError, match="one abundance per sample hash"):
        db.explain_batch(samples, good, abunds=[np.ones(4, np.int64), None])


def test_cohort_device_takes_the_residual_pass_as_an_optional_argument():
    params = inspect.signature(cohort._Device.__init__).parameters
    assert list(params)[:8] == ["self", "db", "covs", "ksize", "ani_thresh", "thr_table", "cap", "abund_samples"]
    assert params["residual_sets"].default == 0
    launch = inspect.signature(cohort._Device.launch).parameters
    assert list(launch)[:3] == ["self", "mins", "abunds"] and all(p.default is None for p in list(launch.values())[2:])
