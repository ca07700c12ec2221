"""RefDB — Python handle over the HIP containment engine (libyacht_hip.so).

A RefDB is a reference-sketch database resident in one GPU's HBM.  It answers the three
questions of YACHT's hot path:

    overlap(sample)              |S ∩ R_j| for every reference       (R1, `yacht run`)
    exclusive(mask, sample)      subset-exclusive hash counts         (R2, `yacht run`)
    pairwise(c_thresh)           above-threshold reference pairs      (T2-T4, `yacht train`)

numpy arrays in, numpy arrays out; all arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import (YH_DB_DEFAULT, YH_DB_KEEP_CSR, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX,  # noqa: F401
                   YH_DB_PAIRWISE_ONLY,
                   YachtHipError)


def pack_csr(sketches: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """Pack a list of ascending uint64 hash arrays into (values, offsets)."""
    offsets = np.zeros(len(sketches) + 1, dtype=np.uint64)
    if len(sketches):
        offsets[1:] = np.cumsum([len(s) for s in sketches], dtype=np.uint64)
    if len(sketches) and int(offsets[-1]):
        values = np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches])
    else:
        values = np.zeros(0, dtype=np.uint64)
    return np.ascontiguousarray(values, dtype=np.uint64), offsets


# one row of the compact result of a run step: a reference with overlap > 0 and its three counts (yh_run_row)
ROW_DTYPE = np.dtype([("ref", np.uint32), ("overlap", np.uint32), ("n_excl", np.uint32), ("n_match", np.uint32)])
# one row of the compact result of a BATCH (yh_batch_row): which sample, which reference, the three counts
BATCH_ROW_DTYPE = np.dtype([("sample", np.uint32), ("ref", np.uint32), ("overlap", np.uint32), ("n_excl", np.uint32),
                            ("n_match", np.uint32)])


def pack_sample(sample, out: Optional[np.ndarray] = None, threads: int = 0) -> np.ndarray:
    """A strictly ascending uint64 sketch as the packed bytes yh_run_submit_packed uploads (~4.7 bytes per hash;
    include/yacht_hip.h).  Host only: no device, any thread.  `out`: a uint8 buffer to pack into (e.g. a
    PinnedArray's array, so that the upload overlaps the kernels); the returned array is the used part of it.
    `threads`: host threads of this one call (0: up to 8 for a large sample; 1: the calling thread only -- for callers
    that pack many samples at once from threads of their own: the C call releases the GIL)."""
    lib = _lib.load()
    sample = _as_u64(sample)
    need = int(lib.yh_sample_pack_bound(sample.size))
    if out is None:
        out = np.empty(need, dtype=np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous
    n = C.c_uint64(0)
    _lib.check(lib.yh_sample_pack_threads(_ptr(sample), sample.size, _ptr(out), out.size, C.byref(n), int(threads)))
    return out[: int(n.value)]


def unpack_sample(packed: np.ndarray) -> np.ndarray:
    """The sketch a packed sample holds (host-side inverse of pack_sample)."""
    lib = _lib.load()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n = C.c_uint64(0)
    _lib.check(lib.yh_sample_unpack(_ptr(packed), packed.size, None, 0, C.byref(n)))
    out = np.zeros(int(n.value), dtype=np.uint64)
    _lib.check(lib.yh_sample_unpack(_ptr(packed), packed.size, _ptr(out), out.size, C.byref(n)))
    return out


def _as_u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def _ptr(a: Optional[np.ndarray]) -> C.c_void_p:
    return C.c_void_p(0 if a is None else a.ctypes.data)


def check_abundances(sample, abund) -> Tuple[np.ndarray, np.ndarray]:
    """(sample as uint64, abund as uint32) for RefDB.abundance, or ValueError: one abundance per sample hash, each in
    [0, 2**32 - 1].  Host only: no library call."""
    sample = _as_u64(sample)
    abund = np.asarray(abund)
    if abund.ndim != 1 or abund.size != sample.size:
        raise ValueError(f"abund must hold one abundance per sample hash: {abund.size} abundances for {sample.size} hashes")
    if abund.size and abund.dtype.kind not in "iu":
        raise ValueError(f"abundances must be integers, not {abund.dtype}")
    if abund.size and (int(abund.max()) > 0xFFFFFFFF or int(abund.min()) < 0):
        raise ValueError("abundances must lie in [0, 2**32 - 1]: the device sums them as 32-bit counts")
    return sample, np.ascontiguousarray(abund, dtype=np.uint32)


def check_member(member, n_refs: int) -> np.ndarray:
    """The member table of RefDB.explain as uint8 [n_refs], or ValueError: one byte per reference, each in [0, 127] (bits
    0..6 are the call sets; bit 7 of a flag means "in the database").  Host only: no library call."""
    member = np.asarray(member)
    if member.ndim != 1 or member.size != int(n_refs):
        raise ValueError(f"member must hold one byte per reference: {member.size} bytes for {int(n_refs)} references")
    if member.size and member.dtype.kind not in "iub":
        raise ValueError(f"member bytes must be integers, not {member.dtype}")
    if member.size and (int(member.max()) > 0x7F or int(member.min()) < 0):
        raise ValueError("member bytes must lie in [0, 127]: bit 7 must be clear, the call sets are bits 0..6")
    return np.ascontiguousarray(member, dtype=np.uint8)


# one row of RefDB.gather (include/yacht_hip.h: yh_gather_row)
GATHER_ROW_DTYPE = np.dtype([("ref", np.uint32), ("n_overlap", np.uint32), ("n_unique", np.uint32), ("reserved_", np.uint32),
                             ("w_unique", np.uint64)])
# one row of RefDB.lca_rows_pack_device (include/yacht_hip.h: yh_lca_row)
LCA_ROW_DTYPE = np.dtype([("sample", np.uint32), ("node", np.uint32), ("n_hashes", np.uint64), ("w_hashes", np.uint64)])
# one row of RefDB.classify_sets (include/yacht_hip.h: yh_classify_row)
CLASSIFY_ROW_DTYPE = np.dtype([("node", np.uint32), ("n_kept", np.uint32), ("n_hit", np.uint32), ("n_root", np.uint32)])
# yh_matrix_cell: one (sample, reference) some coverage calls present; mask = one bit per coverage, depth2 = twice the median depth
MATRIX_CELL_DTYPE = np.dtype([("sample", np.uint32), ("ref", np.uint32), ("n_match", np.uint32), ("mask", np.uint32), ("depth2", np.uint64)])


def check_candidates(cand, n_refs: int) -> np.ndarray:
    """The candidate table of RefDB.gather as uint8 [n_refs] of 0 / 1, or ValueError: one entry per reference, booleans or
    integers (non-zero = candidate).  Host only: no library call."""
    cand = np.asarray(cand)
    if cand.ndim != 1 or cand.size != int(n_refs):
        raise ValueError(f"cand must hold one entry per reference: {cand.size} entries for {int(n_refs)} references")
    if cand.size and cand.dtype.kind not in "iub":
        raise ValueError(f"candidate entries must be booleans or integers, not {cand.dtype}")
    return np.ascontiguousarray(cand != 0, dtype=np.uint8)


def check_gather_limits(min_hits, cap_rows, n_refs: int) -> Tuple[int, int]:
    """(min_hits, cap_rows) of RefDB.gather as integers, or ValueError: min_hits in [1, 2**32 - 1], cap_rows None (no cap:
    a reference wins at most once, so n_refs rows) or >= 0.  Host only: no library call."""
    if int(min_hits) != min_hits or not 1 <= int(min_hits) <= 0xFFFFFFFF:
        raise ValueError(f"min_hits must be an integer in [1, 2**32 - 1], not {min_hits}")
    if cap_rows is None:
        return int(min_hits), int(n_refs)
    if int(cap_rows) != cap_rows or int(cap_rows) < 0:
        raise ValueError(f"cap_rows must be None or an integer >= 0, not {cap_rows}")
    return int(min_hits), min(int(cap_rows), int(n_refs))


def check_gather_batch_limits(cand_mask, min_hits, cap_rows, n_refs: int) -> Tuple[int, int, int]:
    """(cand_mask, min_hits, cap_rows) of RefDB.gather_batch as integers, or ValueError: cand_mask in [1, 255], min_hits in
    [1, 2**32 - 1], cap_rows None (min(n_refs, YH_GATHER_BATCH_MAX_ROWS)) or in [0, YH_GATHER_BATCH_MAX_ROWS]: the rounds of a
    block are enqueued without a host sync, so the cap bounds them.  Host only: no library call."""
    if int(cand_mask) != cand_mask or not 1 <= int(cand_mask) <= 0xFF:
        raise ValueError(f"cand_mask must be an integer in [1, 255], not {cand_mask}")
    if cap_rows is not None and (int(cap_rows) != cap_rows or not 0 <= int(cap_rows) <= _lib.YH_GATHER_BATCH_MAX_ROWS):
        raise ValueError(f"cap_rows must be None or an integer in [0, {_lib.YH_GATHER_BATCH_MAX_ROWS}], not {cap_rows}")
    min_hits, cap = check_gather_limits(min_hits, cap_rows, n_refs)
    return int(cand_mask), min_hits, min(cap, _lib.YH_GATHER_BATCH_MAX_ROWS)


def check_members(members, n_samples: int, n_refs: int) -> np.ndarray:
    """The member rows of RefDB.explain_batch as uint8 [n_samples, n_refs], or ValueError: 1..256 samples, one row per
    sample, one byte per reference, each in [0, 127].  Host only: no library call."""
    if not 1 <= int(n_samples) <= _lib.YH_BATCH_MAX_SAMPLES:
        raise ValueError(f"a block holds 1..{_lib.YH_BATCH_MAX_SAMPLES} samples, not {int(n_samples)}")
    members = np.asarray(members)
    if members.ndim != 2 or members.shape != (int(n_samples), int(n_refs)):
        raise ValueError(f"members must be [n_samples, n_refs] = [{int(n_samples)}, {int(n_refs)}], not {list(members.shape)}")
    if members.size and members.dtype.kind not in "iub":
        raise ValueError(f"member bytes must be integers, not {members.dtype}")
    if members.size and (int(members.max()) > 0x7F or int(members.min()) < 0):
        raise ValueError("member bytes must lie in [0, 127]: bit 7 must be clear, the call sets are bits 0..6")
    return np.ascontiguousarray(members, dtype=np.uint8)


class RefDB:
    """Reference sketches in HBM: delta stream, bucket table + presence filter, shared-hash inverted index."""

    def __init__(self, values, offsets, device: int = 0, flags: int = YH_DB_DEFAULT):
        self._h = C.c_void_p(0)
        lib = _lib.load()
        values = _as_u64(values)
        offsets = _as_u64(offsets)
        if offsets.ndim != 1 or offsets.size < 1:
            raise ValueError("offsets must be a 1-D array of length n_refs + 1")
        if int(offsets[-1]) != values.size:
            raise ValueError("offsets[-1] must equal len(values)")
        h = C.c_void_p(0)
        _lib.check(lib.yh_db_create(_ptr(values), _ptr(offsets), offsets.size - 1, device, flags, C.byref(h)))
        self._h = h
        self._lib = lib
        self.n_refs = offsets.size - 1
        self.sizes = np.diff(offsets).astype(np.uint32)

    @classmethod
    def from_sketches(cls, sketches: Sequence[np.ndarray], **kw) -> "RefDB":
        values, offsets = pack_csr(sketches)
        return cls(values, offsets, **kw)

    @classmethod
    def from_device(cls, d_values: int, d_offsets: int, n_refs: int, sizes: Optional[np.ndarray] = None,
                    device: int = 0, flags: int = YH_DB_DEFAULT) -> "RefDB":
        """Build from CSR arrays that already live in this device's HBM (raw device addresses)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(0)
        lib = _lib.load()
        h = C.c_void_p(0)
        _lib.check(lib.yh_db_create_device(C.c_void_p(d_values), C.c_void_p(d_offsets), n_refs, device, flags, C.byref(h)))
        self._h = h
        self._lib = lib
        self.n_refs = n_refs
        self.sizes = sizes
        return self

    @classmethod
    def from_packed(cls, packed: np.ndarray, sizes: Optional[np.ndarray] = None, device: int = 0, flags: int = YH_DB_DEFAULT) -> "RefDB":
        """Build from a packed CSR (csr_pack's uint64 array): 0.7 of the bytes cross the bus, the sketches are expanded in HBM."""
        assert packed.dtype == np.uint64 and packed.flags["C_CONTIGUOUS"], "csr_pack returns what this takes"
        self = cls.__new__(cls)
        self._h = C.c_void_p(0)
        lib = _lib.load()
        h = C.c_void_p(0)
        _lib.check(lib.yh_db_create_packed(_ptr(packed), packed.nbytes, device, flags, C.byref(h)))
        self._h = h
        self._lib = lib
        self.n_refs = int(self.info()["n_refs"])
        self.sizes = sizes
        return self

    # ---- lifetime ---------------------------------------------------------------------------
    def close(self, release_pool: bool = False) -> None:
        """Destroy the handle.  Its arrays go to the library's buffer cache (the next handle of this process takes them without
        the driver); release_pool=True hands the cache's idle blocks back to the driver as well (_lib.pool_release) -- for a
        process that needs the memory elsewhere next (torch, RCCL)."""
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.yh_db_destroy(h)
            self._h = C.c_void_p(0)
        if release_pool:
            _lib.pool_release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- metadata ---------------------------------------------------------------------------
    def info(self) -> dict:
        inf = _lib.DbInfo()
        _lib.check(self._lib.yh_db_get_info(self._h, C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in inf._fields_}

    def timing(self) -> dict:
        t = _lib.Timing()
        _lib.check(self._lib.yh_db_get_timing(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_}

    def index_stats(self) -> Tuple[int, int, int]:
        """(distinct hashes, hashes in exactly one reference, hashes kept in the index)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.yh_index_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def pairwise_row_stats(self) -> Tuple[int, int]:
        """(rows the last pairwise() summed sparsely, rows it handed back to the dense pass) -- (0, 0): every row dense."""
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.yh_pairwise_row_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_stream(self, hip_stream: int) -> None:
        _lib.check(self._lib.yh_db_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_batch_finish_stream(self, hip_stream: Optional[int]) -> None:
        """The second halves of the batched hash-range calls (run_batch_finish_range_device, words unpack, rows pack) on this
        hipStream_t beside the next block's first half; None = on the handle's stream again (include/yacht_hip.h)."""
        _lib.check(self._lib.yh_db_set_batch_finish_stream(self._h, C.c_void_p(hip_stream or 0)))

    def set_lookup(self, mode: int) -> None:
        """_lib.YH_LOOKUP_AUTO (default: by cost), YH_LOOKUP_STREAM or YH_LOOKUP_INDEXED for overlap / run queries."""
        _lib.check(self._lib.yh_db_set_lookup(self._h, mode))

    def lookup_choice(self, n_sample: int) -> int:
        rc = self._lib.yh_db_lookup_choice(self._h, n_sample)
        if rc < 0:
            _lib.check(rc)
        return rc

    def synchronize(self) -> None:
        _lib.check(self._lib.yh_db_synchronize(self._h))

    # ---- yacht run ---------------------------------------------------------------------------
    def overlap(self, sample, method: str = "tile") -> np.ndarray:
        sample = _as_u64(sample)
        out = np.zeros(self.n_refs, dtype=np.uint32)
        fn = self._lib.yh_overlap if method == "tile" else self._lib.yh_overlap_bsearch
        _lib.check(fn(self._h, _ptr(sample), sample.size, _ptr(out)))
        return out

    def exclusive(self, mask, sample) -> Tuple[np.ndarray, np.ndarray]:
        sample = _as_u64(sample)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.size != self.n_refs:
            raise ValueError("mask must have one entry per reference")
        e = np.zeros(self.n_refs, dtype=np.uint32)
        m = np.zeros(self.n_refs, dtype=np.uint32)
        _lib.check(self._lib.yh_exclusive(self._h, _ptr(mask), _ptr(sample), sample.size, _ptr(e), _ptr(m)))
        return e, m

    def run_counts(self, sample) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """overlap, and exclusive counts relative to the references with overlap > 0."""
        sample = _as_u64(sample)
        ov = np.zeros(self.n_refs, dtype=np.uint32)
        e = np.zeros(self.n_refs, dtype=np.uint32)
        m = np.zeros(self.n_refs, dtype=np.uint32)
        _lib.check(self._lib.yh_run(self._h, _ptr(sample), sample.size, _ptr(ov), _ptr(e), _ptr(m)))
        return ov, e, m

    def abundance(self, sample, abund) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Depth of the sample over every reference (yh_abund): w_overlap[j] = sum of abund over the sample hashes in R_j,
        w_match[j] = the same over the sample hashes whose only holder is j (the set run_counts counts as n_match), both
        uint64, and med_match[j] = the median abundance over that set (float64; 0.0 where it is empty)."""
        sample, abund = check_abundances(sample, abund)
        w_ov = np.zeros(self.n_refs, dtype=np.uint64)
        w_m = np.zeros(self.n_refs, dtype=np.uint64)
        med = np.zeros(self.n_refs, dtype=np.float64)
        _lib.check(self._lib.yh_abund(self._h, _ptr(sample), _ptr(abund), sample.size, _ptr(w_ov), _ptr(w_m), _ptr(med)))
        return w_ov, w_m, med

    def abundance_device(self, d_sample: int, d_abund: int, n_sample: int, d_w_overlap: int, d_w_match: int, d_med: int = 0) -> None:
        """yh_abund_device: uint64 sample and uint32 abundances in, uint64 [N] sums and (d_med != 0) float64 [N] medians out."""
        _lib.check(self._lib.yh_abund_device(self._h, C.c_void_p(d_sample), C.c_void_p(d_abund), n_sample, C.c_void_p(d_w_overlap),
                                             C.c_void_p(d_w_match), C.c_void_p(d_med)))

    def abundance_batch(self, samples: Sequence[np.ndarray], abunds, want_median: bool = True):
        """abundance for a block of 1..256 samples in a fixed number of launches (yh_abund_batch).  abunds: one array per
        sample, one abundance per hash.  Returns (w_overlap, w_match, med_match): uint64 [len(samples), n_refs] twice and
        float64 [len(samples), n_refs] (None with want_median=False: the sums only, without the sort); row s equals
        abundance's for sample s alone."""
        b = len(samples)
        if not 1 <= b <= _lib.YH_BATCH_MAX_SAMPLES:
            raise ValueError(f"a block holds 1..{_lib.YH_BATCH_MAX_SAMPLES} samples, not {b}")
        if len(abunds) != b:
            raise ValueError(f"{len(abunds)} abundance arrays for {b} samples")
        pairs = [check_abundances(s, a) for s, a in zip(samples, abunds)]
        values, offsets = pack_csr([p[0] for p in pairs])
        cat_ab = np.ascontiguousarray(np.concatenate([p[1] for p in pairs]), dtype=np.uint32)
        w_ov = np.zeros((b, self.n_refs), dtype=np.uint64)
        w_m = np.zeros((b, self.n_refs), dtype=np.uint64)
        med = np.zeros((b, self.n_refs), dtype=np.float64) if want_median else None
        _lib.check(self._lib.yh_abund_batch(self._h, _ptr(values), _ptr(offsets), _ptr(cat_ab), b, _ptr(w_ov), _ptr(w_m), _ptr(med)))
        return w_ov, w_m, med

    def abundance_batch_device(self, d_samples: int, d_offsets: int, d_abund: int, n_samples: int, total_hashes: int,
                               d_w_overlap: int, d_w_match: int, d_med: int = 0) -> None:
        """yh_abund_batch_device: the block as for run_batch_device and uint32 abundances beside the hashes in, uint64
        [n_samples][N] sums and (d_med != 0) float64 [n_samples][N] medians out."""
        _lib.check(self._lib.yh_abund_batch_device(self._h, C.c_void_p(d_samples), C.c_void_p(d_offsets), C.c_void_p(d_abund),
                                                   n_samples, total_hashes, C.c_void_p(d_w_overlap), C.c_void_p(d_w_match),
                                                   C.c_void_p(d_med)))

    def explain(self, sample, member, abund=None, want_flags: bool = True) -> Tuple[Optional[np.ndarray], np.ndarray]:
        """What the call sets of `member` explain of the sample (yh_explain).  member: uint8 [n_refs], bit k (0..6) = the
        reference belongs to call set k.  abund: one abundance per sample hash, or None (all 1).  Returns (flags, totals):
        flags uint8 [n], 0 for a hash no reference holds, else 0x80 | OR of the member bytes of all its holders (None with
        want_flags=False: the totals only); totals uint64 [8, 2], per bit the number of sample hashes whose flag has it set
        and the sum of their abundances."""
        if abund is None:
            sample = _as_u64(sample)
        else:
            sample, abund = check_abundances(sample, abund)
        member = check_member(member, self.n_refs)
        flags = np.zeros(sample.size, dtype=np.uint8) if want_flags else None
        totals = np.zeros((8, 2), dtype=np.uint64)
        _lib.check(self._lib.yh_explain(self._h, _ptr(sample), _ptr(abund), sample.size, _ptr(member), _ptr(flags), _ptr(totals)))
        return flags, totals

    def explain_device(self, d_sample: int, d_abund: int, n_sample: int, d_member: int, d_flags: int, d_totals: int) -> None:
        """yh_explain_device: uint64 sample, uint32 abundances (0: all 1) and uint8 [N] member table in, uint8 [n_sample]
        flags (0: none) and uint64 [8][2] totals out."""
        _lib.check(self._lib.yh_explain_device(self._h, C.c_void_p(d_sample), C.c_void_p(d_abund), n_sample, C.c_void_p(d_member),
                                               C.c_void_p(d_flags), C.c_void_p(d_totals)))

    def set_taxonomy(self, parent, depth, leaf) -> None:
        """Hang the references in a taxonomy (yh_db_set_taxonomy): parent uint32 [n_nodes] with parent[0] = 0 and parent[v] <
        v, depth uint8 [n_nodes] with depth[v] = depth[parent[v]] + 1 <= 16, leaf uint32 [n_refs] the node of every reference
        (an internal node or the root, 0, are allowed).  Synchronous; replaces an earlier taxonomy; parent=None (or no
        node) removes it.  A tree the library refuses raises YachtHipError (YH_ERR_INVALID_ARG) and the earlier one stays."""
        if parent is None or np.asarray(parent).size == 0:
            _lib.check(self._lib.yh_db_set_taxonomy(self._h, None, None, 0, None))
            return
        parent, depth, leaf = np.asarray(parent), np.asarray(depth), np.asarray(leaf)
        if parent.ndim != 1 or depth.shape != parent.shape:
            raise ValueError(f"parent and depth must hold one entry per node: {list(parent.shape)} and {list(depth.shape)}")
        if leaf.ndim != 1 or leaf.size != self.n_refs:
            raise ValueError(f"leaf must hold one node per reference: {leaf.size} entries for {self.n_refs} references")
        for name, a, top in (("parent", parent, 0xFFFFFFFF), ("depth", depth, 0xFF), ("leaf", leaf, 0xFFFFFFFF)):
            if a.dtype.kind not in "iu":
                raise ValueError(f"{name} must be integers, not {a.dtype}")
            if a.size and (int(a.min()) < 0 or int(a.max()) > top):
                raise ValueError(f"{name} must lie in [0, {top}]")
        if parent.size >= 0xFFFFFFFF:
            raise ValueError("a taxonomy holds fewer than 2**32 - 1 nodes")
        parent = np.ascontiguousarray(parent, dtype=np.uint32)
        depth = np.ascontiguousarray(depth, dtype=np.uint8)
        leaf = np.ascontiguousarray(leaf, dtype=np.uint32)
        _lib.check(self._lib.yh_db_set_taxonomy(self._h, _ptr(parent), _ptr(depth), parent.size, _ptr(leaf)))

    def taxonomy_info(self) -> dict:
        """{"n_nodes": nodes of the taxonomy set (0: none), "device_bytes": what its arrays take} (yh_db_get_taxonomy)."""
        n, b = C.c_uint32(0), C.c_uint64(0)
        _lib.check(self._lib.yh_db_get_taxonomy(self._h, C.byref(n), C.byref(b)))
        return {"n_nodes": int(n.value), "device_bytes": int(b.value)}

    def lca(self, sample, abund=None, want_nodes: bool = True) -> Tuple[Optional[np.ndarray], np.ndarray]:
        """Every sample hash classified by the lowest common ancestor of its holders in the taxonomy (yh_lca).  abund: one
        abundance per sample hash, or None (all 1).  Returns (nodes, counts): nodes uint32 [n], _lib.YH_LCA_NONE for a hash
        no reference holds, else the node of its only holder or the LCA of all of them (None with want_nodes=False: the
        counts only); counts uint64 [n_nodes, 2], per node the number of sample hashes that resolve exactly there and the sum
        of their abundances (direct assignments: taxonomy.clade_sums adds the subtrees)."""
        if abund is None:
            sample = _as_u64(sample)
        else:
            sample, abund = check_abundances(sample, abund)
        nodes = np.full(sample.size, _lib.YH_LCA_NONE, dtype=np.uint32) if want_nodes else None
        counts = np.zeros((self.taxonomy_info()["n_nodes"], 2), dtype=np.uint64)
        _lib.check(self._lib.yh_lca(self._h, _ptr(sample), _ptr(abund), sample.size, _ptr(nodes), _ptr(counts)))
        return nodes, counts

    def lca_device(self, d_sample: int, d_abund: int, n_sample: int, d_node: int, d_counts: int) -> None:
        """yh_lca_device: uint64 sample and uint32 abundances (0: all 1) in, uint32 [n_sample] nodes (0: none) and uint64
        [n_nodes][2] counts out."""
        _lib.check(self._lib.yh_lca_device(self._h, C.c_void_p(d_sample), C.c_void_p(d_abund), n_sample, C.c_void_p(d_node),
                                           C.c_void_p(d_counts)))

    def lca_batch(self, samples: Sequence[np.ndarray], abunds=None, want_nodes: bool = True):
        """lca for a block of 1..256 samples in one lookup launch (yh_lca_batch).  abunds: None (all 1) or one entry per
        sample, each an array of one abundance per hash or None (that sample's hashes count once).  Returns (nodes, counts):
        nodes a list of uint32 arrays, one per sample (None with want_nodes=False), counts uint64 [len(samples), n_nodes, 2];
        both equal lca's for each sample alone."""
        b = len(samples)
        if not 1 <= b <= _lib.YH_BATCH_MAX_SAMPLES:
            raise ValueError(f"a block holds 1..{_lib.YH_BATCH_MAX_SAMPLES} samples, not {b}")
        samples = [_as_u64(s) for s in samples]
        cat_ab = None
        if abunds is not None:
            if len(abunds) != b:
                raise ValueError(f"{len(abunds)} abundance arrays for {b} samples")
            if any(a is not None for a in abunds):
                parts = [np.ones(s.size, dtype=np.uint32) if a is None else check_abundances(s, a)[1] for s, a in zip(samples, abunds)]
                cat_ab = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint32)
        values, offsets = pack_csr(samples)
        nodes = np.full(values.size, _lib.YH_LCA_NONE, dtype=np.uint32) if want_nodes else None
        counts = np.zeros((b, self.taxonomy_info()["n_nodes"], 2), dtype=np.uint64)
        _lib.check(self._lib.yh_lca_batch(self._h, _ptr(values), _ptr(offsets), _ptr(cat_ab), b, _ptr(nodes), _ptr(counts)))
        return ([nodes[int(offsets[s]):int(offsets[s + 1])] for s in range(b)] if want_nodes else None), counts

    def lca_batch_device(self, d_samples: int, d_offsets: int, d_abund: int, n_samples: int, total_hashes: int, d_node: int,
                         d_counts: int) -> None:
        """yh_lca_batch_device: the block as for explain_batch_device and uint32 abundances (0: all 1) in, uint32
        [total_hashes] nodes (0: none) and uint64 [n_samples][n_nodes][2] counts out.  Does not synchronize the host."""
        _lib.check(self._lib.yh_lca_batch_device(self._h, C.c_void_p(d_samples), C.c_void_p(d_offsets), C.c_void_p(d_abund),
                                                 n_samples, total_hashes, C.c_void_p(d_node), C.c_void_p(d_counts)))

    def lca_rows_pack_device(self, d_counts: int, n_samples: int, d_rows: int, cap_rows: int, d_n_rows: int) -> None:
        """yh_lca_rows_pack_device: the non-zero cells of uint64 [n_samples][n_nodes][2] counts as rows of LCA_ROW_DTYPE in
        (sample, node) order, the first cap_rows of them, and their true number as one uint64 at d_n_rows (device).  Does not
        synchronize the host."""
        if int(cap_rows) < 0:
            raise ValueError(f"cap_rows must be >= 0, not {cap_rows}")
        _lib.check(self._lib.yh_lca_rows_pack_device(self._h, C.c_void_p(d_counts), n_samples, C.c_void_p(d_rows), int(cap_rows),
                                                     C.c_void_p(d_n_rows)))

    # ---- a taxon for every record (yh_classify.hip; yacht_amd.classify drives it) --------------------------------------------
    def classify_sets(self, mins, off, want_nodes: bool = False):
        """One row per set of the CSR (mins, off[n_sets + 1]) under the taxonomy set (yh_classify_sets): set s owns
        mins[off[s]:off[s + 1]], strictly ascending inside the set.  Returns rows, a structured array of CLASSIFY_ROW_DTYPE
        [n_sets]: node = the LCA of the set's informative hits (those whose node is neither _lib.YH_LCA_NONE nor the root), 0
        with hits but none informative, YH_LCA_NONE without a hit; n_kept, n_hit, n_root the set's entries, those some
        reference holds, and those that resolve to the root.  With want_nodes=True: (rows, nodes), nodes uint32 [len(mins)]
        as RefDB.lca gives them for each set alone."""
        mins = _as_u64(mins)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("off needs n_sets + 1 entries")
        if int(off[-1]) != mins.size:
            raise ValueError(f"off ends at {int(off[-1])}, mins holds {mins.size} entries")
        rows = np.zeros(off.size - 1, dtype=CLASSIFY_ROW_DTYPE)
        nodes = np.full(mins.size, _lib.YH_LCA_NONE, dtype=np.uint32) if want_nodes else None
        _lib.check(self._lib.yh_classify_sets(self._h, _ptr(mins), _ptr(off), off.size - 1, _ptr(rows), _ptr(nodes)))
        return (rows, nodes) if want_nodes else rows

    def classify_sets_device(self, d_mins: int, d_off: int, n_sets: int, total: int, d_rows: int, d_node: int = 0) -> None:
        """yh_classify_sets_device: uint64 mins and uint64 [n_sets + 1] offsets in (total: the host's copy of the last offset),
        CLASSIFY_ROW_DTYPE [n_sets] rows and uint32 [total] nodes (0: none) out.  Does not synchronize the host."""
        _lib.check(self._lib.yh_classify_sets_device(self._h, C.c_void_p(d_mins), C.c_void_p(d_off), int(n_sets), int(total),
                                                     C.c_void_p(d_rows), C.c_void_p(d_node)))

    def classify_segments(self, buf, seg_off, ksize: int, scaled: int, seed: int = 42, return_total: bool = False):
        """One row of CLASSIFY_ROW_DTYPE per segment of `buf` (yh_classify_segments): every segment sketched as
        sketch.sketch_segments does and its sketch classified as classify_sets does, with the sketches staying on the device.
        seg_off [n_seg + 1]: ascending byte offsets from 0 to len(buf).  `scaled` must be the database's own: the caller
        answers for it.  return_total=True: (rows, the entries of all sketches)."""
        from .sketch import max_hash_for_scaled
        if isinstance(buf, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(buf, dtype=np.uint8)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(seg_off, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("seg_off needs n_seg + 1 entries")
        rows = np.zeros(off.size - 1, dtype=CLASSIFY_ROW_DTYPE)
        n = C.c_uint64(0)
        _lib.check(self._lib.yh_classify_segments(self._h, _ptr(buf) if buf.size else None, buf.size, _ptr(off), off.size - 1, int(ksize),
                                                  int(seed), max_hash_for_scaled(scaled), _ptr(rows), C.byref(n)))
        return (rows, int(n.value)) if return_total else rows

    # ---- the organism x sample tables of a cohort (yh_matrix.hip; yacht_amd.matrix drives them) ----------------------------
    def matrix_cells_device(self, d_rows: int, d_n_rows: int, cap_rows: int, d_present: int, n_sets: int, d_med: int, sample_base: int,
                            d_cells: int, d_n_cells: int) -> None:
        """yh_matrix_cells_device: the block's compact rows, their count (device), uint8 [n_sets][cap_rows] present bytes and
        float64 [cap_rows] medians (0: none) in; the rows some coverage calls present as cells of MATRIX_CELL_DTYPE in row
        order and their number as one uint64 at d_n_cells (device) out.  Does not synchronize the host."""
        _lib.check(self._lib.yh_matrix_cells_device(self._h, C.c_void_p(d_rows), C.c_void_p(d_n_rows), int(cap_rows), C.c_void_p(d_present),
                                                    int(n_sets), C.c_void_p(d_med), int(sample_base), C.c_void_p(d_cells),
                                                    C.c_void_p(d_n_cells)))

    def matrix_prevalence_device(self, d_cells: int, n_cells: int, n_sets: int, n_samples: int, d_skip: int, d_prev: int,
                                 d_denom: int) -> None:
        """yh_matrix_prevalence_device: uint32 [n_sets][N] samples-present counts and uint64 [n_sets][n_samples] sums of depth2
        of the cells (cleared first); d_skip: uint8 [n_samples] or 0.  Does not synchronize the host."""
        _lib.check(self._lib.yh_matrix_prevalence_device(self._h, C.c_void_p(d_cells), int(n_cells), int(n_sets), int(n_samples),
                                                         C.c_void_p(d_skip), C.c_void_p(d_prev), C.c_void_p(d_denom)))

    def matrix_fill_device(self, d_cells: int, n_cells: int, bit: int, n_samples: int, d_skip: int, d_row_of_ref: int, n_kept: int,
                           d_denom_bit: int, d_presence: int, d_n_match: int, d_rel: int) -> None:
        """yh_matrix_fill_device: the [n_kept][n_samples] matrices of coverage `bit` (uint8 presence, uint32 n_match, float64
        relative abundance or 0 for none), cleared first; d_row_of_ref: int32 [N], -1 for a dropped reference.  Does not
        synchronize the host."""
        _lib.check(self._lib.yh_matrix_fill_device(self._h, C.c_void_p(d_cells), int(n_cells), int(bit), int(n_samples), C.c_void_p(d_skip),
                                                   C.c_void_p(d_row_of_ref), int(n_kept), C.c_void_p(d_denom_bit), C.c_void_p(d_presence),
                                                   C.c_void_p(d_n_match), C.c_void_p(d_rel)))

    def gather(self, sample, cand, abund=None, min_hits: int = 1, cap_rows: Optional[int] = None, want_owner: bool = False):
        """The candidates ranked by the sample hashes each adds (yh_gather): round after round the candidate holding the
        most sample hashes nobody owns yet (ties: the smallest index) takes them.  cand: one byte per reference, non-zero =
        candidate.  abund: one abundance per sample hash, or None (all 1).  cap_rows: at most this many rows (None: no
        cap).  Returns (rows, more, owner): rows a structured array (GATHER_ROW_DTYPE: ref, n_overlap, n_unique, w_unique),
        more True when the cap cut the run short of a candidate with min_hits live hashes, owner uint32 [n] with
        0xFFFFFFFF = nobody (None without want_owner)."""
        if abund is None:
            sample = _as_u64(sample)
        else:
            sample, abund = check_abundances(sample, abund)
        cand = check_candidates(cand, self.n_refs)
        min_hits, cap = check_gather_limits(min_hits, cap_rows, self.n_refs)
        rows = np.zeros(max(cap, 1), dtype=GATHER_ROW_DTYPE)
        owner = np.full(sample.size, _lib.YH_GATHER_NOBODY, dtype=np.uint32) if want_owner else None
        n_rows, more = C.c_uint64(0), C.c_int(0)
        _lib.check(self._lib.yh_gather(self._h, _ptr(sample), _ptr(abund), sample.size, _ptr(cand), min_hits, _ptr(rows), cap,
                                       _ptr(owner), C.byref(n_rows), C.byref(more)))
        return rows[:int(n_rows.value)].copy(), bool(more.value), owner

    def gather_device(self, d_sample: int, d_abund: int, n_sample: int, d_cand: int, min_hits: int, d_rows: int, cap_rows: int,
                      d_owner: int = 0) -> Tuple[int, bool]:
        """yh_gather_device: uint64 sample, uint32 abundances (0: all 1) and uint8 [N] candidate table in, cap_rows rows
        of GATHER_ROW_DTYPE and (d_owner != 0) uint32 [n_sample] owners out.  Synchronizes the handle's stream once per
        chunk of rounds.  Returns (n_rows, more)."""
        n_rows, more = C.c_uint64(0), C.c_int(0)
        _lib.check(self._lib.yh_gather_device(self._h, C.c_void_p(d_sample), C.c_void_p(d_abund), n_sample, C.c_void_p(d_cand),
                                              int(min_hits), C.c_void_p(d_rows), int(cap_rows), C.c_void_p(d_owner),
                                              C.byref(n_rows), C.byref(more)))
        return int(n_rows.value), bool(more.value)

    def gather_batch(self, samples: Sequence[np.ndarray], members, cand_mask: int = 1, abunds=None, min_hits: int = 1,
                     cap_rows: Optional[int] = None, want_owner: bool = False):
        """gather for a block of 1..256 samples in the same launches (yh_gather_batch).  members: uint8 [len(samples),
        n_refs]; reference j is a candidate of sample s when members[s, j] & cand_mask is non-zero (the member rows of
        explain_batch, one bit per call set).  abunds: as for explain_batch.  cap_rows: at most this many rows per sample,
        None = min(n_refs, YH_GATHER_BATCH_MAX_ROWS), never above that maximum.  Returns (rows, more, owners): a list of
        GATHER_ROW_DTYPE arrays, a list of booleans and a list of uint32 owner arrays (None without want_owner), each equal
        to gather's for that sample alone."""
        b = len(samples)
        if not 1 <= b <= _lib.YH_BATCH_MAX_SAMPLES:
            raise ValueError(f"a block holds 1..{_lib.YH_BATCH_MAX_SAMPLES} samples, not {b}")
        members = np.asarray(members)
        if members.ndim != 2 or members.shape != (b, self.n_refs):
            raise ValueError(f"members must be [n_samples, n_refs] = [{b}, {self.n_refs}], not {list(members.shape)}")
        if members.size and members.dtype.kind not in "iub":
            raise ValueError(f"member bytes must be integers, not {members.dtype}")
        members = np.ascontiguousarray(members, dtype=np.uint8)
        cand_mask, min_hits, cap = check_gather_batch_limits(cand_mask, min_hits, cap_rows, self.n_refs)
        samples = [_as_u64(s) for s in samples]
        cat_ab = None
        if abunds is not None:
            if len(abunds) != b:
                raise ValueError(f"{len(abunds)} abundance arrays for {b} samples")
            if any(a is not None for a in abunds):
                parts = [np.ones(s.size, dtype=np.uint32) if a is None else check_abundances(s, a)[1] for s, a in zip(samples, abunds)]
                cat_ab = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint32)
        values, offsets = pack_csr(samples)
        rows = np.zeros((b, max(cap, 1)), dtype=GATHER_ROW_DTYPE)
        owner = np.full(values.size, _lib.YH_GATHER_NOBODY, dtype=np.uint32) if want_owner else None
        n_rows, more = np.zeros(b, dtype=np.uint32), np.zeros(b, dtype=np.uint8)
        _lib.check(self._lib.yh_gather_batch(self._h, _ptr(values), _ptr(offsets), _ptr(cat_ab), b, _ptr(members), cand_mask, min_hits,
                                             _ptr(rows), cap, _ptr(owner), _ptr(n_rows), _ptr(more)))
        return ([rows[s, :int(n_rows[s])].copy() for s in range(b)], [bool(m) for m in more],
                [owner[int(offsets[s]):int(offsets[s + 1])] for s in range(b)] if want_owner else None)

    def gather_batch_device(self, d_samples: int, d_offsets: int, d_abund: int, n_samples: int, total_hashes: int, d_members: int,
                            cand_mask: int, min_hits: int, d_rows: int, cap_rows: int, d_owner: int, d_n_rows: int, d_more: int) -> None:
        """yh_gather_batch_device: the block as for explain_batch_device, uint32 abundances (0: all 1) and uint8 [n_samples][N]
        member rows in; [n_samples][cap_rows] rows of GATHER_ROW_DTYPE, uint32 [total_hashes] owners (0: none), uint32
        [n_samples] row counts and uint8 [n_samples] `more` bytes out, all on the device.  Does not synchronize the host."""
        if not 1 <= int(cand_mask) <= 0xFF:
            raise ValueError(f"cand_mask must be an integer in [1, 255], not {cand_mask}")
        if not 0 <= int(min_hits) <= 0xFFFFFFFF or int(cap_rows) < 0:
            raise ValueError(f"min_hits must lie in [0, 2**32 - 1] and cap_rows be >= 0, not {min_hits} and {cap_rows}")
        _lib.check(self._lib.yh_gather_batch_device(self._h, C.c_void_p(d_samples), C.c_void_p(d_offsets), C.c_void_p(d_abund),
                                                    n_samples, total_hashes, C.c_void_p(d_members), int(cand_mask), int(min_hits),
                                                    C.c_void_p(d_rows), int(cap_rows), C.c_void_p(d_owner), C.c_void_p(d_n_rows),
                                                    C.c_void_p(d_more)))

    def explain_batch(self, samples: Sequence[np.ndarray], members, abunds=None, want_flags: bool = True):
        """explain for a block of 1..256 samples, each with its own member row, in one lookup launch (yh_explain_batch).
        members: uint8 [len(samples), n_refs], row s the member table of sample s.  abunds: None (all 1) or one entry per
        sample, each an array of one abundance per hash or None (that sample's hashes count once).  Returns (flags, totals):
        flags a list of uint8 arrays, one per sample (None with want_flags=False), totals uint64 [len(samples), 8, 2];
        both equal explain's for each sample alone."""
        b = len(samples)
        members = check_members(members, b, self.n_refs)
        samples = [_as_u64(s) for s in samples]
        cat_ab = None
        if abunds is not None:
            if len(abunds) != b:
                raise ValueError(f"{len(abunds)} abundance arrays for {b} samples")
            if any(a is not None for a in abunds):
                parts = [np.ones(s.size, dtype=np.uint32) if a is None else check_abundances(s, a)[1] for s, a in zip(samples, abunds)]
                cat_ab = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint32) if parts else None
        values, offsets = pack_csr(samples)
        flags = np.zeros(values.size, dtype=np.uint8) if want_flags else None
        totals = np.zeros((b, 8, 2), dtype=np.uint64)
        _lib.check(self._lib.yh_explain_batch(self._h, _ptr(values), _ptr(offsets), _ptr(cat_ab), b, _ptr(members), _ptr(flags),
                                              _ptr(totals)))
        return ([flags[int(offsets[s]):int(offsets[s + 1])] for s in range(b)] if want_flags else None), totals

    def explain_batch_device(self, d_samples: int, d_offsets: int, d_abund: int, n_samples: int, total_hashes: int, d_members: int,
                             d_flags: int, d_totals: int) -> None:
        """yh_explain_batch_device: the block as for run_batch_device, uint32 abundances beside the hashes (0: all 1) and
        uint8 [n_samples][N] member rows in, uint8 [total_hashes] flags (0: none) and uint64 [n_samples][8][2] totals out."""
        _lib.check(self._lib.yh_explain_batch_device(self._h, C.c_void_p(d_samples), C.c_void_p(d_offsets), C.c_void_p(d_abund),
                                                     n_samples, total_hashes, C.c_void_p(d_members), C.c_void_p(d_flags),
                                                     C.c_void_p(d_totals)))

    def explain_members_rows_device(self, d_rows: int, d_n_rows: int, cap_rows: int, d_present: int, n_sets: int, n_samples: int,
                                    d_members: int) -> None:
        """yh_explain_members_rows_device: the block's compact rows, their count (device) and uint8 [n_sets][cap_rows] present
        bytes in, uint8 [n_samples][N] member rows out (cleared first)."""
        _lib.check(self._lib.yh_explain_members_rows_device(self._h, C.c_void_p(d_rows), C.c_void_p(d_n_rows), cap_rows,
                                                            C.c_void_p(d_present), n_sets, n_samples, C.c_void_p(d_members)))

    # sharded run (dist.ShardedRefDB): the step in two halves around the exchange of the subset bits
    def set_ghosts(self, ghost_begin: int, n_ghost: int, d_ghost_src: int) -> None:
        _lib.check(self._lib.yh_db_set_ghosts(self._h, ghost_begin, n_ghost, C.c_void_p(d_ghost_src)))

    def run_local_device(self, d_sample: int, n_sample: int, d_overlap: int, d_excl: int, d_match: int,
                         d_bits_out: int, ctx: int = 0) -> None:
        _lib.check(self._lib.yh_run_local_device(self._h, ctx, C.c_void_p(d_sample), n_sample, C.c_void_p(d_overlap),
                                                 C.c_void_p(d_excl), C.c_void_p(d_match), C.c_void_p(d_bits_out)))

    def run_finish_device(self, d_global_bits: int, d_excl: int, ctx: int = 0) -> None:
        _lib.check(self._lib.yh_run_finish_device(self._h, ctx, C.c_void_p(d_global_bits), C.c_void_p(d_excl)))

    # hash-range shards (dist.HashRangeRefDB): the step in two halves around the all-gather of the ranks' subset bits
    def run_local_range_device(self, d_sample: int, n_sample: int, d_overlap: int, d_match: int, d_bits_out: int,
                               ctx: int = 0) -> None:
        _lib.check(self._lib.yh_run_local_range_device(self._h, ctx, C.c_void_p(d_sample), n_sample, C.c_void_p(d_overlap),
                                                       C.c_void_p(d_match), C.c_void_p(d_bits_out)))

    def run_finish_range_device(self, d_gathered_bits: int, n_ranks: int, stride_words: int, d_excl: int, ctx: int = 0) -> None:
        _lib.check(self._lib.yh_run_finish_range_device(self._h, ctx, C.c_void_p(d_gathered_bits), n_ranks, stride_words,
                                                        C.c_void_p(d_excl)))

    def run_batch_local_range_device(self, d_samples: int, d_offsets: int, n_samples: int, total_hashes: int, d_overlap: int,
                                     d_maskwords_out: int, slot: int = 0) -> None:
        _lib.check(self._lib.yh_run_batch_local_range_device(self._h, slot, C.c_void_p(d_samples), C.c_void_p(d_offsets), n_samples,
                                                             total_hashes, C.c_void_p(d_overlap), C.c_void_p(d_maskwords_out)))

    def run_batch_finish_range_device(self, n_samples: int, d_gathered: int, n_ranks: int, d_overlap: int, d_excl: int,
                                      d_match: int, slot: int = 0) -> None:
        _lib.check(self._lib.yh_run_batch_finish_range_device(self._h, slot, n_samples, C.c_void_p(d_gathered), n_ranks,
                                                              C.c_void_p(d_overlap), C.c_void_p(d_excl), C.c_void_p(d_match)))

    # the compact form of a batch's result: one entry per (reference, sample) of the batch's subset, in (reference, sample) order
    def run_batch_rows_pack_device(self, d_overlap: int, d_excl: int, d_match: int, d_vals: int, cap_rows: int, d_n_rows: int,
                                   slot: int = 0) -> None:
        """d_vals [cap_rows][3] uint32 = this handle's (overlap, n_excl, n_match) of every entry; d_n_rows: their number."""
        _lib.check(self._lib.yh_run_batch_rows_pack_device(self._h, slot, C.c_void_p(d_overlap), C.c_void_p(d_excl), C.c_void_p(d_match),
                                                           C.c_void_p(d_vals), cap_rows, C.c_void_p(d_n_rows)))

    def run_batch_rows_unpack_device(self, d_vals: int, cap_rows: int, d_rows: int, d_n_rows: int, slot: int = 0) -> None:
        """d_rows [cap_rows] BATCH_ROW_DTYPE = (sample, ref, overlap, n_excl, n_match) from (summed) values."""
        _lib.check(self._lib.yh_run_batch_rows_unpack_device(self._h, slot, C.c_void_p(d_vals), cap_rows, C.c_void_p(d_rows),
                                                             C.c_void_p(d_n_rows)))

    # the subset words of a block in compact form: what a hash-range rank all-gathers between the two halves
    def run_batch_words_pack_device(self, d_words: int, d_packed: int, cap_words: int, n_planes: int = 1) -> None:
        """d_packed [words_packed_len(cap_words)] uint64 = count, the non-zero words of d_words [n_planes][N], their ids
        (plane * N + reference); n_planes = batch_planes(samples of the block)."""
        _lib.check(self._lib.yh_run_batch_words_pack_device(self._h, C.c_void_p(d_words), n_planes, C.c_void_p(d_packed), cap_words))

    def run_batch_words_unpack_device(self, d_gathered: int, n_ranks: int, cap_words: int, d_words_out: int, d_overflow: int,
                                      n_planes: int = 1) -> None:
        """d_words_out [n_planes][N] uint64 = OR of the n_ranks packed buffers at d_gathered; d_overflow [1] uint32 = some rank overflowed."""
        _lib.check(self._lib.yh_run_batch_words_unpack_device(self._h, C.c_void_p(d_gathered), n_ranks, n_planes, cap_words,
                                                              C.c_void_p(d_words_out), C.c_void_p(d_overflow)))

    def run_submit(self, slot: int, sample: np.ndarray, overlap: np.ndarray, n_excl: np.ndarray,
                   n_match: np.ndarray) -> None:
        """Queue one `yacht run` count call (upload, ordering check, kernels, download) without waiting;
        run_wait(slot) completes it.  Arrays must stay alive (and unchanged) until then; page-locked
        arrays (pinned_empty) make the copies overlap the kernels of the neighbouring calls."""
        assert sample.dtype == np.uint64 and sample.flags.c_contiguous
        for a in (overlap, n_excl, n_match):
            assert a.dtype == np.uint32 and a.flags.c_contiguous and a.size >= self.n_refs
        _lib.check(self._lib.yh_run_submit(self._h, slot, _ptr(sample), sample.size, _ptr(overlap), _ptr(n_excl),
                                           _ptr(n_match)))

    def run_wait(self, slot: int) -> None:
        _lib.check(self._lib.yh_run_wait(self._h, slot))

    def run_submit_packed(self, slot: int, packed: np.ndarray, rows: np.ndarray) -> None:
        """Queue one run step from a packed sample (pack_sample); its result comes back as compact rows -- one
        ROW_DTYPE record per reference with overlap > 0 -- in `rows`; run_wait_rows(slot) returns how many."""
        assert packed.dtype == np.uint8 and packed.flags.c_contiguous
        assert rows.dtype == ROW_DTYPE and rows.flags.c_contiguous
        _lib.check(self._lib.yh_run_submit_packed(self._h, slot, _ptr(packed), packed.size, _ptr(rows), rows.size))

    def run_submit_rows(self, slot: int, sample: np.ndarray, rows: np.ndarray) -> None:
        assert sample.dtype == np.uint64 and sample.flags.c_contiguous
        assert rows.dtype == ROW_DTYPE and rows.flags.c_contiguous
        _lib.check(self._lib.yh_run_submit_rows(self._h, slot, _ptr(sample), sample.size, _ptr(rows), rows.size))

    def run_wait_rows(self, slot: int) -> int:
        n = C.c_uint64(0)
        _lib.check(self._lib.yh_run_wait_rows(self._h, slot, C.byref(n)))
        return int(n.value)

    def run_rows(self, sample, packed: bool = True) -> np.ndarray:
        """run_counts as compact rows (ROW_DTYPE, ascending by reference): only the references with overlap > 0."""
        sample = _as_u64(sample)
        cap = max(1024, self.n_refs // 16)
        while True:
            rows = np.zeros(cap, dtype=ROW_DTYPE)
            if packed:
                self.run_submit_packed(0, pack_sample(sample), rows)
            else:
                self.run_submit_rows(0, sample, rows)
            n = C.c_uint64(0)
            rc = self._lib.yh_run_wait_rows(self._h, 0, C.byref(n))
            if rc == _lib.YH_ERR_CAPACITY:
                cap = int(n.value)
                continue
            _lib.check(rc)
            return rows[: int(n.value)]

    def run_rows_device(self, d_overlap: int, d_excl: int, d_match: int, d_rows: int, cap_rows: int, d_n_rows: int) -> None:
        _lib.check(self._lib.yh_run_rows_device(self._h, C.c_void_p(d_overlap), C.c_void_p(d_excl), C.c_void_p(d_match),
                                                C.c_void_p(d_rows), cap_rows, C.c_void_p(d_n_rows)))

    def run_batch(self, samples: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """run_counts for up to BATCH_MAX_SAMPLES (256) samples in one pass (needs the directory: not YH_DB_NO_DIRECTORY): three uint32
        arrays of shape [len(samples), n_refs]."""
        values, offsets = pack_csr(samples)
        b = len(samples)
        out = [np.zeros((b, self.n_refs), dtype=np.uint32) for _ in range(3)]
        _lib.check(self._lib.yh_run_batch(self._h, _ptr(values), _ptr(offsets), b, *(_ptr(a) for a in out)))
        return out[0], out[1], out[2]

    def run_batch_device(self, d_samples: int, d_offsets: int, n_samples: int, total_hashes: int, d_overlap: int,
                         d_excl: int, d_match: int) -> None:
        _lib.check(self._lib.yh_run_batch_device(self._h, C.c_void_p(d_samples), C.c_void_p(d_offsets), n_samples,
                                                 total_hashes, C.c_void_p(d_overlap), C.c_void_p(d_excl),
                                                 C.c_void_p(d_match)))

    # device-pointer forms (async on the handle's stream; raw addresses, e.g. tensor.data_ptr())
    def overlap_device(self, d_sample: int, n_sample: int, d_overlap: int) -> None:
        _lib.check(self._lib.yh_overlap_device(self._h, C.c_void_p(d_sample), n_sample, C.c_void_p(d_overlap)))

    def overlap_bsearch_device(self, d_sample: int, n_sample: int, d_overlap: int) -> None:
        _lib.check(self._lib.yh_overlap_bsearch_device(self._h, C.c_void_p(d_sample), n_sample,
                                                       C.c_void_p(d_overlap)))

    def overlap_indexed_device(self, d_sample: int, n_sample: int, d_overlap: int) -> None:
        _lib.check(self._lib.yh_overlap_indexed_device(self._h, C.c_void_p(d_sample), n_sample, C.c_void_p(d_overlap)))

    def run_indexed_device(self, d_sample: int, n_sample: int, d_overlap: int, d_excl: int, d_match: int) -> None:
        _lib.check(self._lib.yh_run_indexed_device(self._h, C.c_void_p(d_sample), n_sample, C.c_void_p(d_overlap),
                                                   C.c_void_p(d_excl), C.c_void_p(d_match)))

    def run_device(self, d_sample: int, n_sample: int, d_overlap: int, d_excl: int = 0, d_match: int = 0) -> None:
        _lib.check(self._lib.yh_run_device(self._h, C.c_void_p(d_sample), n_sample, C.c_void_p(d_overlap),
                                           C.c_void_p(d_excl), C.c_void_p(d_match)))

    def run_device_pipelined(self, d_sample: int, n_sample: int, d_overlap: int, d_excl: int, d_match: int) -> None:
        """run_device whose tail runs beside the next call's lookup; outputs are complete after run_device_join()
        (or any other query / synchronize on the handle).  Alternate at least two output buffers."""
        _lib.check(self._lib.yh_run_device_pipelined(self._h, C.c_void_p(d_sample), n_sample, C.c_void_p(d_overlap),
                                                     C.c_void_p(d_excl), C.c_void_p(d_match)))

    def run_device_join(self) -> None:
        _lib.check(self._lib.yh_run_device_join(self._h))

    # ---- yacht train -------------------------------------------------------------------------
    def nshared_device(self, d_out: int) -> None:
        """d_out[j] = shared hashes of reference j (device array of n_refs uint32): the row weights of the pairwise pass."""
        _lib.check(self._lib.yh_db_nshared_device(self._h, C.c_void_p(d_out)))

    def pairwise(self, c_thresh: float, row_begin: int = 0, row_end: Optional[int] = None):
        """Ordered pairs (i, j, |R_i ∩ R_j|) with !(count/|R_i| < c_thresh), sorted by (i, j)."""
        if row_end is None:
            row_end = self.n_refs
        n = C.c_uint64(0)
        _lib.check(self._lib.yh_pairwise(self._h, c_thresh, row_begin, row_end, 0, None, None, None, C.byref(n)))
        cap = max(int(n.value), 1)
        pi = np.zeros(cap, dtype=np.uint32)
        pj = np.zeros(cap, dtype=np.uint32)
        pc = np.zeros(cap, dtype=np.uint32)
        _lib.check(self._lib.yh_pairwise(self._h, c_thresh, row_begin, row_end, cap, _ptr(pi), _ptr(pj), _ptr(pc),
                                         C.byref(n)))
        k = int(n.value)
        return pi[:k], pj[:k], pc[:k]


BATCH_MAX_SAMPLES = 256  # include/yacht_hip.h: YH_BATCH_MAX_SAMPLES


def batch_planes(n_samples: int) -> int:
    """Planes of 64 samples the subset words of a batch take (include/yacht_hip.h: YH_BATCH_PLANES)."""
    return (int(n_samples) + 63) // 64


def csr_pack(values: np.ndarray, offsets: np.ndarray, threads: int = 0) -> np.ndarray:
    """A CSR of strictly ascending uint64 sketches -> the packed form yh_db_create_packed / RefDB.from_packed take (a uint64
    array: 8-byte aligned); ~5.7 bytes per hash for sketches of ~5 000 hashes at scaled = 1000."""
    lib = _lib.load()
    values = np.ascontiguousarray(values, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    need = C.c_uint64(0)
    _lib.check(lib.yh_csr_pack(_ptr(values), _ptr(offsets), n, None, 0, C.byref(need), threads))
    out = np.zeros((int(need.value) + 7) // 8, dtype=np.uint64)
    _lib.check(lib.yh_csr_pack(_ptr(values), _ptr(offsets), n, _ptr(out), out.nbytes, C.byref(need), threads))
    assert int(need.value) == out.nbytes
    return out


def csr_subset(packed: np.ndarray, rows: Sequence[int]) -> np.ndarray:
    """The listed sketches of a packed CSR, in that order, as a packed CSR of their own (yh_csr_subset: no hash is decoded)."""
    lib = _lib.load()
    assert packed.dtype == np.uint64 and packed.flags["C_CONTIGUOUS"]
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    need = C.c_uint64(0)
    _lib.check(lib.yh_csr_subset(_ptr(packed), packed.nbytes, _ptr(rows), rows.size, None, 0, C.byref(need)))
    out = np.zeros((int(need.value) + 7) // 8, dtype=np.uint64)
    _lib.check(lib.yh_csr_subset(_ptr(packed), packed.nbytes, _ptr(rows), rows.size, _ptr(out), out.nbytes, C.byref(need)))
    return out


def packed_offsets(packed: np.ndarray) -> np.ndarray:
    """The offsets[N + 1] a packed CSR carries behind its 64-byte header (a view: header word 1 = N)."""
    n = int(packed[1])
    return packed[8: 8 + n + 1]


def csr_unpack(packed: np.ndarray):
    """(values, offsets) of a packed CSR, on the host."""
    lib = _lib.load()
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    h, n = C.c_uint64(0), C.c_uint64(0)
    _lib.check(lib.yh_csr_unpack(_ptr(packed), packed.nbytes, None, 0, None, 0, C.byref(h), C.byref(n)))
    values = np.zeros(max(int(h.value), 1), dtype=np.uint64)
    offsets = np.zeros(int(n.value) + 1, dtype=np.uint64)
    _lib.check(lib.yh_csr_unpack(_ptr(packed), packed.nbytes, _ptr(values), int(h.value), _ptr(offsets), int(n.value), C.byref(h), C.byref(n)))
    return values[:int(h.value)], offsets


class PinnedArray:
    """A page-locked host array (yh_host_alloc) viewed as numpy; freed with the object."""

    def __init__(self, n: int, dtype):
        lib = _lib.load()
        self._lib = lib
        dt = np.dtype(dtype)
        p = C.c_void_p(0)
        _lib.check(lib.yh_host_alloc(C.byref(p), max(int(n) * dt.itemsize, 16)))
        self._p = p
        buf = (C.c_uint8 * (int(n) * dt.itemsize)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dt, count=int(n))

    def close(self) -> None:
        if self._p is not None and self._p.value:
            self.array = None
            self._lib.yh_host_free(self._p)
            self._p = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_select(sizes, pair_i, pair_j) -> np.ndarray:
    """Greedy size-ordered dedup (src/cpp/main.cpp:371-407): kept reference ids in walk order."""
    lib = _lib.load()
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    pair_i = np.ascontiguousarray(pair_i, dtype=np.uint32)
    pair_j = np.ascontiguousarray(pair_j, dtype=np.uint32)
    sel = np.zeros(max(sizes.size, 1), dtype=np.uint32)
    n = C.c_uint64(0)
    _lib.check(lib.yh_train_select(_ptr(sizes), sizes.size, _ptr(pair_i), _ptr(pair_j), pair_i.size, _ptr(sel),
                                   C.byref(n)))
    return sel[: int(n.value)]
