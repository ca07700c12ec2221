"""The batched abundance pass without a GPU: the oracle alone (tests/abund_oracle.py) shows that the edge block of
abund_batch_cases.py holds, at the tile's edges, enough of every kind of (sample, reference) pair a batched median can get
wrong; the header declares the two entries (the ABI stays 8), the library exports them and refuses a null handle and a
bad block size, and the binding types them."""
import ctypes as C
import os

import numpy as np
import pytest
from abund_batch_cases import EDGE_SIZES, T, abundances, edge_block, edge_classes

from yacht_amd import _lib, cohort, engine

ENTRIES = ("yh_abund_batch_device", "yh_abund_batch")


def test_the_edge_block_sits_on_the_edges_that_matter():
    samples, abunds, want, counts = edge_block()
    assert [s.size for s in samples] == EDGE_SIZES == [0, 1, T - 1, T, T + 1, 2 * T + 1, 3000, 5 * T + 7]
    for s, (smp, ab) in enumerate(zip(samples, abunds)):
        assert ab.size == smp.size and (smp.size < 2 or bool((np.diff(smp.astype(np.int64)) > 0).all()))
        if smp.size > 1:
            assert int(ab.min()) >= 1 and int(ab.max()) <= (1000 if s % 2 == 0 else 50)
    got = edge_classes()
    print(got)
    # at least 50 pairs with exactly one and exactly two exclusive hits, with an odd count from 3, with a median that ends
    # in .5, and with 0 < w_match < w_overlap; at least 50 references whose medians differ between the 2 T + 1 and the 5 T + 7 sample
    assert min(got.values()) >= 50, got
    for s in range(len(samples)):  # every median is x.0 or x.5, 0.0 exactly where no hit is exclusive
        med = want[s][2]
        assert bool(((med * 2) % 1.0 == 0).all()) and np.array_equal(med > 0, counts[s] > 0)


def test_odd_samples_have_many_equal_abundances():
    rng = np.random.default_rng(5)
    even, odd = abundances(rng, 0, 4000), abundances(rng, 1, 4000)
    assert even.dtype == odd.dtype == np.uint32 and np.unique(even).size > 900 and np.unique(odd).size < 30 and int(odd.max()) <= 50


def test_header_declares_the_entries_and_the_abi_stays_8():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert f"int {name}(" in text, name
    assert "#define YH_ABI_VERSION 8" in text
    table = text[text.index("entry point   "):text.index("#define YH_RUN_CONTEXTS")]
    assert "yh_abund_batch / yh_abund_batch_device" in table
    assert f"#define YH_ABUND_BATCH_TILE {_lib.YH_ABUND_BATCH_TILE}\n" in text


def test_binding_types_the_entries():
    assert [len(_lib.SIGNATURES[name][1]) for name in ENTRIES] == [9, 8]
    for name in ("abundance_batch_device", "abundance_batch"):
        assert callable(getattr(engine.RefDB, name))
    assert callable(cohort._Device.abundance_pass)


def test_library_exports_the_entries_and_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.yh_abi_version() == 8
    for name in ENTRIES:
        assert hasattr(lib, name), name
    buf = np.zeros(64, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.yh_abund_batch_device(None, p, p, p, 1, 0, p, p, None) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_abund_batch(None, p, p, p, 1, p, p, None) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()


def test_abundance_batch_checks_its_arguments_before_any_library_call():
    db = engine.RefDB.__new__(engine.RefDB)  # no handle: the checks come before any library call
    db._h = C.c_void_p(0)
    db.n_refs = 3
    samples = [np.arange(1, 6, dtype=np.uint64), np.zeros(0, np.uint64)]
    with pytest.raises(ValueError, match="1..256 samples"):
        db.abundance_batch([], [])
    with pytest.raises(ValueError, match="1..256 samples"):
        db.abundance_batch([samples[0]] * 257, [np.ones(5, np.int64)] * 257)
    with pytest.raises(ValueError, match="abundance arrays"):
        db.abundance_batch(samples, [np.ones(5, np.int64)])
    with pytest.raises(ValueError, match="one abundance per sample hash"):
        db.abundance_batch(samples, [np.ones(4, np.int64), np.zeros(0, np.int64)])
