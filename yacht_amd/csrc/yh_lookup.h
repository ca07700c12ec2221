// yh_lookup.h — the ONE place the distinct-hash directory (YhDirView, yh_common.h) is probed from by the tile kernels:
// k_index_lookup_tile / k_step_fused (yh_query.hip: lookup_tile_body), k_abund_lookup / k_abund_batch_lookup (yh_abund.hip),
// k_explain_lookup (yh_explain.hip) and k_batch_lookup (yh_batch.hip).  Device code, plus the host-side table of the tile shapes.
//
// A lane holds U sample hashes h[u] with ok[u] = "still worth looking up".  A hash that is not (past the sample's end, or
// above the database's largest hash) is set to 0 by the kernel: 0 is still a valid filter word and bucket to read, so
// the loads below need no branch around them.  The probe is three stages, and the kernels do work of their own between
// them (table clear in front of the filter, __syncthreads() between request and resolve): that order is measured.
//   1. yh_probe_filter   one presence-filter word per hash, ALL words requested before any is looked at
//   2. yh_probe_request  the compact bucket of every hash still ok, all loads in flight, then the fence
//   3. yh_probe_resolve  the dref word of hash u (holder id, or 0x80000000 | shared-hash index), or YH_DIR_NONE
// What a hit MEANS (+1, += abundance, OR of member bytes) stays in each kernel.
#pragma once
#include "yh_common.h"

// ---- the tile shape for a sample size (host) -------------------------------------------------------
// THREADS lanes x U hashes per workgroup, 2^TBITS slots in the LDS hit table.  Small samples are latency-bound: 256-lane
// workgroups keep every CU busy, and no filter word is read in front of the bucket.  Once there are enough tiles for
// every CU, 1024-lane tiles of one, then two hashes per lane (step time on the bench database by sample size:
// yh_q_overlap_indexed).  Every launch site switches over `form` to its own template instantiations of exactly these
// numbers; form 3 is never chosen by size (YH_INDEX_TILE=4, the stand-alone lookup's tuning shape).
struct YhTileShape {
    int form;      // 0 = <1, 256, 8>, 1 = <1, 1024, 10>, 2 = <2, 1024, 10>, 3 = <4, 1024, 10>
    int U;
    u32 threads;
    int tbits;
    bool filter;   // the presence filter is read (where the handle has one: yh_filter_of)
    u32 tiles(u64 n_sample) const { return (u32)((n_sample + (u64)threads * U - 1) / ((u64)threads * U)); }
};
inline YhTileShape yh_tile_shape(int form) {
    static const YhTileShape shapes[4] = {{0, 1, 256u, 8, false}, {1, 1, 1024u, 10, true}, {2, 2, 1024u, 10, true}, {3, 4, 1024u, 10, true}};
    return shapes[form];
}
inline YhTileShape yh_tile_shape_for(u64 n_sample) {
    return yh_tile_shape(n_sample >= 512ull * 1024 ? 2 : n_sample >= 256ull * 1024 ? 1 : 0);
}

#if defined(__HIPCC__)
template <int U>
struct YhProbe {
    YhDirView::v4u a[U], b[U], c[U], d[U];  // the four 16-byte words of each hash's compact bucket
};

// Stage 1.  A hash whose filter bits are clear is not in the database (yh_db::d_filter); one whose bits are set may
// still be absent, so the filter only ever turns ok[u] OFF and never decides a hit: counts stay exact.  filter == null
// (no filter, or a shape that reads none): nothing happens.
template <int U>
__device__ __forceinline__ void yh_probe_filter(const YhDirView& dv, const u32* __restrict__ filter, u64 filter_mul,
                                                const u64 (&h)[U], bool (&ok)[U]) {
    if (!filter) return;
    u64 bit[U];
    u32 w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        bit[u] = yh_bucket_of(h[u], dv.bkt_lsh, filter_mul);
        w[u] = filter[bit[u] >> 5];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const u32 m = yh_filter_mask(h[u], bit[u]);
        ok[u] = ok[u] && (w[u] & m) == m;
    }
}

// Stage 2.  Without compact buckets (dv.cbkt == null) nothing happens: stage 3 then takes YhDirView::find.  The empty
// asm is a fence: all four loads of every bucket are issued, unconditionally, before anything looks at them.  Left to
// itself the compiler sinks the loads of w[0] / w[8] under "entries > 0", which it only knows after the first loads
// have come back -- a second dependent memory round trip per lookup (55 us instead of 30 for 10^6 lookups).
template <int U>
__device__ __forceinline__ void yh_probe_request(const YhDirView& dv, const u64 (&h)[U], const bool (&ok)[U], YhProbe<U>& p) {
    if (!dv.cbkt) return;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        p.a[u] = p.b[u] = p.c[u] = p.d[u] = YhDirView::v4u{0u, 0u, 0u, 0u};
        if (ok[u]) dv.cbkt_request(h[u], p.a[u], p.b[u], p.c[u], p.d[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) asm volatile("" : "+v"(p.a[u]), "+v"(p.b[u]), "+v"(p.c[u]), "+v"(p.d[u]));
}

// Stage 3.
template <int U>
__device__ __forceinline__ u32 yh_probe_resolve(const YhDirView& dv, const u64 (&h)[U], const bool (&ok)[U], const YhProbe<U>& p, int u) {
    if (!ok[u]) return YH_DIR_NONE;
    return dv.cbkt ? dv.cbkt_resolve(h[u], p.a[u], p.b[u], p.c[u], p.d[u]) : dv.find(h[u]);
}

// a workgroup-uniform value read from LDS, back in scalar registers (the loop state of a tile then costs no vector registers)
__device__ __forceinline__ u64 uniform64(u64 v) {
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}

// The slot of reference `ref` in a workgroup's LDS hit table of 2^TBITS keys (tkey: reference + 1, 0 = empty), claimed
// with at most two probes; -1 when both are taken by other references (a crowded table: the caller adds to global
// memory directly).  What is summed at the slot is the caller's.
template <int TBITS>
__device__ __forceinline__ int yh_hit_slot(u32* tkey, u32 ref) {
    constexpr u32 TSLOTS = 1u << TBITS;
    u32 slot = (ref * 2654435761u) >> (32 - TBITS);
#pragma unroll 1
    for (int probe = 0; probe < 2; ++probe, slot = (slot + 1) & (TSLOTS - 1)) {
        const u32 old = atomicCAS(&tkey[slot], 0u, ref + 1);
        if (old == 0 || old == ref + 1) return (int)slot;
    }
    return -1;
}

// The posting list of a shared hash found in the sample: add(holder) for every holder.  The holders are requested four
// at a time (a list of 8 was 8 dependent round trips: the tail of the launch for a sample of cluster members).
template <typename Add>
__device__ __forceinline__ void walk_holders(const u64* __restrict__ po, const u32* __restrict__ pr, u32 gi, Add add) {
    const u64 q0 = po[gi], qe = po[gi + 1];
    for (u64 q = q0; q < qe; q += 4) {
        u32 h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (q + (u64)i < qe) add(h[i]);
    }
}
#endif
