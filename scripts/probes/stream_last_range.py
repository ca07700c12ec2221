#!/usr/bin/env python3
"""GPU box: the streaming lookup asked with sample hashes above the database's largest key, far apart (DESIGN.md 3,
k_stream_lookup).  A database of three stream blocks (3 072 consecutive hashes, shift 0) and a sample of six of its hashes
plus N hashes above max_hash, 2^33 apart; the stream lookup forced; one call to warm up on the six hits alone (handle set-up),
then one timed call of overlap and one of run_counts.  Prints one JSON line.  usage: stream_last_range.py N
(YACHT_HIP_LIB selects the library)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yacht_amd import _lib  # noqa: E402
from yacht_amd.engine import RefDB  # noqa: E402

n_far = int(sys.argv[1])
hashes = np.arange(1000, 1000 + 3072, dtype=np.uint64)
refs = np.arange(3072) % 8
order = np.lexsort((hashes, refs))
values = hashes[order]
offsets = np.concatenate([[0], np.cumsum(np.bincount(refs, minlength=8))]).astype(np.uint64)
hits = hashes[[0, 1, 1023, 1024, 2125, 3071]]
far = np.uint64(hashes[-1]) + (np.arange(1, n_far + 1, dtype=np.uint64) << np.uint64(33))
sample = np.concatenate([hits, far])
want = np.bincount(refs[[0, 1, 1023, 1024, 2125, 3071]], minlength=8)
with RefDB(values, offsets) as db:
    db.set_lookup(_lib.YH_LOOKUP_STREAM)
    assert db.lookup_choice(sample.size) == _lib.YH_LOOKUP_STREAM
    assert np.array_equal(db.overlap(hits), want)
    t0 = time.perf_counter()
    ov = db.overlap(sample)
    t1 = time.perf_counter()
    ov2, _e, _m = db.run_counts(sample)
    t2 = time.perf_counter()
    assert np.array_equal(ov, want) and np.array_equal(ov2, want)
print(json.dumps({"library": os.path.basename(_lib.lib_path()), "hashes_above_max_hash": n_far, "overlap_seconds": round(t1 - t0, 4),
                  "run_counts_seconds": round(t2 - t1, 4), "counts": "right"}))
