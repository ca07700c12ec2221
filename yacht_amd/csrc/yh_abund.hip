// yh_abund.hip — per-reference DEPTH of a sample with per-hash abundances (yh_abund_device, include/yacht_hip.h).
//
// For a sample S (strictly ascending) with abundances a(h) and every reference j:
//   w_overlap[j] = sum of a(h) over h in S ∩ R_j
//   w_match[j]   = sum of a(h) over the h in S whose ONLY holder in the database is j
//   med_match[j] = median of a(h) over that same set (even count: mean of the two middle values; empty: 0.0)
//
// Why "only holder in the database" is the set yh_run counts as n_match: n_match[j] counts the hashes of R_j that are in
// the sample and in no OTHER reference of the run subset (overlap > 0).  A sample hash held by j and k gives both of
// them overlap, so both are in the subset: a SAMPLE hash is exclusive to j exactly when j is its only holder in the
// database -- its dref word has the top bit clear (YhDirView::find).  The same holds for any superset of the subset.
// So this pass needs no subset bits, no step context, no batch slot and no exclusive work list: it is the directory
// probe of yh_lookup.h with "+= a(h)" in place of the indexed lookup's "+= 1", and the posting list of a shared hash
// feeds w_overlap only.  (With ghosts registered exclusivity is not local to the handle: the entry refuses.)
//
// Layout: k_abund_lookup (tiles of THREADS x U sample hashes, all filter reads then all bucket reads in flight, hits summed
// per reference in an LDS table that leaves as one 64-bit atomic per (workgroup, reference, sum): integer adds, so the
// result does not depend on arrival order; the single-holder hits appended to a hit buffer, one counter atomic per
// workgroup) -> rocprim::radix_sort_keys over the (reference << 32 | a) keys of those hits -> k_abund_median (one lane per reference, two lower-bound searches).  The last two only when the
// caller asks for the median.  yh_abund_batch_device answers a BLOCK of samples with a fixed number of launches: further down.
#include "yh_abund.h"
#include "yh_lookup.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>

namespace {

struct AbundLookup {
    const u64* sample;
    const u32* abund;
    u64 n;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u64* po;
    const u32* pr;
    u64* w_overlap;
    u64* w_match;
    u64* keys;     // [n] (reference << 32) | a of every single-holder hit, in arrival order; null: no median wanted
    u64* n_hits;   // [1] keys appended so far (one atomic per workgroup)
};

// (tkey: reference + 1, 0 = empty; tov / tmt: the two sums of that reference in this workgroup's tile)
template <int U, int THREADS, int TBITS>
__global__ void __launch_bounds__(THREADS) k_abund_lookup(const AbundLookup q) {
    constexpr u32 TSLOTS = 1u << TBITS;
    __shared__ u32 tkey[TSLOTS];
    __shared__ u64 tov[TSLOTS];
    __shared__ u64 tmt[TSLOTS];
    __shared__ u32 wg_hits;   // single-holder hits of this workgroup
    __shared__ u64 wg_first;  // ... and their first place in the hit buffer
    const u64* __restrict__ sample = q.sample;
    const u32* __restrict__ abund = q.abund;
    const u64 n = q.n;
    const YhDirView& dv = q.dv;
    const u32* __restrict__ filter = q.filter;
    const u64 base = blockIdx.x * (u64)(THREADS * U);
    u64 h[U];
    u32 ab[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const u64 t = base + (u64)u * THREADS + threadIdx.x;
        const u64 tc = min(t, n - 1);  // (n >= 1: the launch has no workgroup otherwise)
        h[u] = sample[tc];
        ab[u] = abund[tc];
        ok[u] = t < n && h[u] <= dv.max_hash;
        if (!ok[u]) h[u] = 0;  // (still a valid bucket to read)
    }
    for (u32 k = threadIdx.x; k < TSLOTS; k += THREADS) { tkey[k] = 0; tov[k] = 0; tmt[k] = 0; }
    if (threadIdx.x == 0) wg_hits = 0;
    YhProbe<U> probe;
    u32 r[U];
    yh_probe_filter<U>(dv, filter, q.filter_mul, h, ok);
    yh_probe_request<U>(dv, h, ok, probe);
    __syncthreads();  // the table is clear
    auto add = [&](u32 ref, u64 v, bool only_holder) {
        const int slot = yh_hit_slot<TBITS>(tkey, ref);
        if (slot >= 0) {
            atomicAdd(&tov[slot], v);
            if (only_holder) atomicAdd(&tmt[slot], v);
            return;
        }
        atomicAdd(&q.w_overlap[ref], v);  // crowded table: sum directly
        if (only_holder) atomicAdd(&q.w_match[ref], v);
    };
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = yh_probe_resolve<U>(dv, h, ok, probe, u);
    // The places of the single-holder hits in the hit buffer, aggregated twice: a wave's hits take consecutive places
    // (ballot; one returning LDS atomic per wave), and the workgroup claims all of its places with ONE returning global
    // atomic on the device counter.  (One global atomic per wave -- 15 600 of them on one address for a 10^6-hash sample,
    // serialized memory-side -- made this kernel 210 us instead of 40: profiles/abund/kernel_stats.txt.)
    const u32 lane = threadIdx.x & 63u;
    u32 place[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool single = r[u] != YH_DIR_NONE && !(r[u] & 0x80000000u);
        place[u] = 0;
        if (q.keys) {  // (uniform)
            const u64 votes = __ballot(single);
            if (votes) {
                const int leader = __ffsll((long long)votes) - 1;
                u32 first = 0;
                if ((int)lane == leader) first = atomicAdd(&wg_hits, (u32)__popcll(votes));
                first = (u32)__shfl((int)first, leader);
                place[u] = first + (u32)__popcll(votes & ((1ull << lane) - 1ull));
            }
        }
        if (single) {
            add(r[u], ab[u], true);
        } else if (r[u] != YH_DIR_NONE) {
            const u64 v = ab[u];
            walk_holders(q.po, q.pr, r[u] & 0x7fffffffu, [&](u32 holder) { add(holder, v, false); });
        }
    }
    __syncthreads();
    if (q.keys && threadIdx.x == 0 && wg_hits) wg_first = atomicAdd(q.n_hits, (u64)wg_hits);
    for (u32 k = threadIdx.x; k < TSLOTS; k += THREADS)
        if (tkey[k]) {
            atomicAdd(&q.w_overlap[tkey[k] - 1], tov[k]);
            if (tmt[k]) atomicAdd(&q.w_match[tkey[k] - 1], tmt[k]);
        }
    if (!q.keys) return;  // (uniform)
    __syncthreads();
    // (a sample hash appends at most once: at most n keys in all)
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (r[u] != YH_DIR_NONE && !(r[u] & 0x80000000u)) q.keys[wg_first + place[u]] = ((u64)r[u] << 32) | ab[u];
}

// the output arrays cleared in ONE launch (two or three hipMemsetAsync are a launch each); c may be null
__global__ void __launch_bounds__(256) k_abund_clear(u64* __restrict__ a, u64* __restrict__ b, u64* __restrict__ c, u64 n) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        a[i] = 0;
        b[i] = 0;
        if (c) c[i] = 0;
    }
}

// first index of keys[0, n) whose key is >= x
__device__ __forceinline__ u64 abund_lower_bound(const u64* __restrict__ keys, u64 n, u64 x) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// keys[0, n): the hit keys ascending, the unused tail all ones (above every key of a reference: ids stay below 2^31)
__global__ void __launch_bounds__(256) k_abund_median(const u64* __restrict__ keys, u64 n, u64 n_refs, double* __restrict__ med) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= n_refs) return;
    const u64 lo = abund_lower_bound(keys, n, j << 32);
    const u64 hi = abund_lower_bound(keys, n, (j + 1) << 32);
    const u64 cnt = hi - lo;
    double m = 0.0;
    if (cnt) {
        const u64 up = lo + cnt / 2;
        const u32 x1 = (u32)keys[up];
        m = (cnt & 1) ? (double)x1 : 0.5 * ((double)(u32)keys[up - 1] + (double)x1);
    }
    med[j] = m;
}

// ---- the same for a BLOCK of samples (yh_abund_batch_device) ------------------------------------------------------------------
// k_abund_batch_clear -> k_abund_batch_lookup -> rocprim::segmented_radix_sort_keys -> k_abund_batch_median (+ k_abund_batch_median_spilled,
// which has no work unless total_hashes was too small): a fixed number of launches whatever n_samples is.
// A workgroup's unit of work is a tile of AB_TILE consecutive hashes of ONE sample in k_explain_batch_lookup's slot order (the
// resident workgroups share a stretch of the hash range across samples), so the tile's sample is workgroup-uniform: the LDS hit
// table of k_abund_lookup lives for the tile's four rounds and leaves as 64-bit atomics into row s.  The single-holder hits are
// staged in LDS (a wave's hits take consecutive places: a ballot and one returning LDS atomic per wave and round), and the
// tile claims its places in the sample's OWN segment of the key buffer with ONE returning atomic on seg_end[s] -- which starts
// at off[s] (k_abund_batch_clear), so that it ends up as the end offset of the segment's used part, what the segmented sort
// and the median kernel take.  A sample appends at most its own length: segment s stays inside [off[s], off[s + 1]).
// total_hashes is the caller's number and sizes the key buffer (cap): a sample whose segment would pass it -- only with a
// total_hashes below the device offsets' -- appends nothing, its segment stays empty, and k_abund_batch_median_spilled finds
// its medians without a key buffer.
// (71 VGPRs, no vector spill, 20.5 KB of LDS: seven waves per SIMD by registers, and seven workgroups = 28 waves per CU by LDS
// -- the same seven per SIMD; k_explain_batch_lookup has 79 and six.)
constexpr u32 AB_TILE = YH_ABUND_BATCH_TILE;  // (include/yacht_hip.h)
constexpr u32 AB_THREADS = 256;
constexpr int AB_TBITS = 9;
constexpr u32 AB_MAX = 256;  // samples per block (include/yacht_hip.h: YH_BATCH_MAX_SAMPLES)
static_assert(AB_TILE % AB_THREADS == 0, "a tile is whole rounds of the workgroup");

struct AbundBatch {
    const u64* samples;
    const u64* soff;   // [n_samples + 1]
    const u32* abund;  // [total]
    u32 n_samples;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u64* po;
    const u32* pr;
    u64 n_refs;
    u64* w_overlap;  // [n_samples][n_refs], cleared in front of the lookup
    u64* w_match;
    u64* keys;       // [cap] (reference << 32) | a of the single-holder hits, sample s in its segment; null: no median wanted
    u32* seg_end;    // [n_samples] end of the used part of segment s; k_abund_batch_clear leaves min(off[s], cap) here
    u64 cap;         // total_hashes as the caller gave it (< 2^32 when keys != null)
};

// The three outputs cleared in ONE launch (c may be null), and the segments of the key buffer opened: seg[0][s] = seg[1][s] =
// min(off[s], cap) (seg may be null).  The clamp keeps a segment that lies behind the key buffer empty AND inside it.
__global__ void __launch_bounds__(256) k_abund_batch_clear(u64* __restrict__ a, u64* __restrict__ b, u64* __restrict__ c, u64 n,
                                                           const u64* __restrict__ soff, u32 n_samples, u64 cap, u32* __restrict__ seg) {
    const u64 i0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    for (u64 i = i0; i < n; i += (u64)gridDim.x * blockDim.x) {
        a[i] = 0;
        b[i] = 0;
        if (c) c[i] = 0;
    }
    if (seg && i0 < n_samples) seg[i0] = seg[n_samples + i0] = (u32)min(soff[i0], cap);
}

// the dref word of sample hash k of [base, base + n) when ONE reference holds it, else YH_DIR_NONE; every lane of the workgroup calls
__device__ __forceinline__ u32 abund_single_holder(const AbundBatch& q, u64 base, u64 n, u64 k) {
    u64 h[1] = {q.samples[base + min(k, n - 1)]};
    bool ok[1] = {k < n && h[0] <= q.dv.max_hash};
    if (!ok[0]) h[0] = 0;  // (still a valid word / bucket to read)
    YhProbe<1> probe;
    yh_probe_filter<1>(q.dv, q.filter, q.filter_mul, h, ok);
    yh_probe_request<1>(q.dv, h, ok, probe);
    const u32 r = yh_probe_resolve<1>(q.dv, h, ok, probe, 0);
    return (r & 0x80000000u) ? YH_DIR_NONE : r;
}

__global__ void __launch_bounds__(AB_THREADS) k_abund_batch_lookup(const AbundBatch q) {
    constexpr u32 TSLOTS = 1u << AB_TBITS;
    __shared__ u64 off[AB_MAX + 1];
    __shared__ u64 s_max_nt;
    __shared__ u32 tkey[TSLOTS];  // (reference + 1, 0 = empty; tov / tmt: the two sums of that reference in this tile)
    __shared__ u64 tov[TSLOTS];
    __shared__ u64 tmt[TSLOTS];
    __shared__ u64 stage[AB_TILE];  // the tile's keys before they have a place in the key buffer
    __shared__ u32 wg_hits;         // single-holder hits of this tile
    __shared__ u32 wg_first;        // ... and their first place in the key buffer
    const u64* __restrict__ samples = q.samples;
    const u32* __restrict__ abund = q.abund;
    const YhDirView& dv = q.dv;
    const u32* __restrict__ filter = q.filter;
    const u32 n_samples = q.n_samples;
    for (u32 k = threadIdx.x; k <= n_samples; k += AB_THREADS) off[k] = q.soff[k];
    if (threadIdx.x == 0) s_max_nt = 0;
    __syncthreads();
    {   // the longest sample's tiles (one wave: a maximum over <= 256 lengths)
        u64 m = 0;
        if (threadIdx.x < 64)
            for (u32 k = threadIdx.x; k < n_samples; k += 64) m = max(m, (off[k + 1] - off[k] + AB_TILE - 1) / AB_TILE);
        if (threadIdx.x < 64 && m) atomicMax((unsigned long long*)&s_max_nt, (unsigned long long)m);
    }
    __syncthreads();
    const u64 max_nt = uniform64(s_max_nt);
    const u32 lane = threadIdx.x & 63u;
    // k_explain_batch_lookup's order: slot (v, s) is tile i = v * nt_s / max_nt of sample s; inside a group of 8 quantile steps x
    // n_samples slots, workgroup l takes step l % 8 of sample l / 8
    const u64 n_slots = max_nt * n_samples;
    const u64 group = 8ull * n_samples;
    for (u64 c = blockIdx.x; c < (n_slots + group - 1) / group * group; c += gridDim.x) {  // (workgroup-uniform)
        const u64 l = c % group;
        const u64 v = (c / group) * 8 + (l & 7u);
        const u32 s = (u32)(l >> 3);
        if (v >= max_nt) continue;
        const u64 base = uniform64(off[s]);
        const u64 end = uniform64(off[s + 1]);
        const u64 n_s = end - base, nt_s = (n_s + AB_TILE - 1) / AB_TILE;
        if (nt_s == 0) continue;
        const u64 i = v * nt_s / max_nt;
        if (v > 0 && (v - 1) * nt_s / max_nt == i) continue;  // (a shorter sample: this tile had its slot already)
        for (u32 k = threadIdx.x; k < TSLOTS; k += AB_THREADS) { tkey[k] = 0; tov[k] = 0; tmt[k] = 0; }
        if (threadIdx.x == 0) wg_hits = 0;
        __syncthreads();
        const bool keep = q.keys && end <= q.cap;  // (workgroup-uniform) the sample's segment lies inside the key buffer
        u64* __restrict__ w_overlap = q.w_overlap + (u64)s * q.n_refs;
        u64* __restrict__ w_match = q.w_match + (u64)s * q.n_refs;
        auto add = [&](u32 ref, u64 val, bool only_holder) {
            const int slot = yh_hit_slot<AB_TBITS>(tkey, ref);
            if (slot >= 0) {
                atomicAdd(&tov[slot], val);
                if (only_holder) atomicAdd(&tmt[slot], val);
                return;
            }
            atomicAdd(&w_overlap[ref], val);  // crowded table: sum directly
            if (only_holder) atomicAdd(&w_match[ref], val);
        };
        const u64 k_end = min(n_s, (i + 1) * AB_TILE);
        for (u64 k0 = i * AB_TILE; k0 < k_end; k0 += AB_THREADS) {  // (workgroup-uniform)
            const u64 k = k0 + threadIdx.x;
            const u64 t = base + min(k, k_end - 1);
            u64 h[1] = {samples[t]};
            const u32 ab = abund[t];
            bool ok[1] = {k < k_end && h[0] <= dv.max_hash};
            if (!ok[0]) h[0] = 0;  // (still a valid word / bucket to read)
            YhProbe<1> probe;
            yh_probe_filter<1>(dv, filter, q.filter_mul, h, ok);
            yh_probe_request<1>(dv, h, ok, probe);
            const u32 r = yh_probe_resolve<1>(dv, h, ok, probe, 0);
            const bool single = r != YH_DIR_NONE && !(r & 0x80000000u);
            if (keep) {  // (uniform) a hash appends at most once: at most AB_TILE keys in stage
                const u64 votes = __ballot(single);
                if (votes) {
                    const int leader = __ffsll((long long)votes) - 1;
                    u32 first = 0;
                    if ((int)lane == leader) first = atomicAdd(&wg_hits, (u32)__popcll(votes));
                    first = (u32)__shfl((int)first, leader);
                    if (single) stage[first + (u32)__popcll(votes & ((1ull << lane) - 1ull))] = ((u64)r << 32) | ab;
                }
            }
            if (single) {
                add(r, ab, true);
            } else if (r != YH_DIR_NONE) {
                const u64 val = ab;
                walk_holders(q.po, q.pr, r & 0x7fffffffu, [&](u32 holder) { add(holder, val, false); });
            }
        }
        __syncthreads();
        if (threadIdx.x == 0 && wg_hits) wg_first = atomicAdd(&q.seg_end[s], wg_hits);
        for (u32 k = threadIdx.x; k < TSLOTS; k += AB_THREADS)
            if (tkey[k]) {
                atomicAdd(&w_overlap[tkey[k] - 1], tov[k]);
                if (tmt[k]) atomicAdd(&w_match[tkey[k] - 1], tmt[k]);
            }
        __syncthreads();
        // (wg_first + k < off[s] + n_s <= cap by the count above; the comparison costs nothing and holds for any offsets)
        for (u32 k = threadIdx.x; k < wg_hits; k += AB_THREADS)
            if ((u64)wg_first + k < q.cap) q.keys[(u64)wg_first + k] = stage[k];
        __syncthreads();  // (the table and the stage are cleared for the next slot)
    }
}

// One lane per place of the key buffer.  A place inside the used part of a segment (seg_begin[s] <= i < seg_end[s]) whose key
// opens a run of one reference -- the segment's first key, or another reference than the key in front -- finds the run's end
// with ONE search and stores its median into the cleared med[s][reference]: only runs that exist do work.
__global__ void __launch_bounds__(256) k_abund_batch_median(const u64* __restrict__ keys, const u32* __restrict__ seg, u32 n_samples,
                                                            u64 cap, u64 n_refs, double* __restrict__ med) {
    __shared__ u32 sbegin[AB_MAX], send[AB_MAX];
    for (u32 k = threadIdx.x; k < n_samples; k += blockDim.x) { sbegin[k] = seg[k]; send[k] = seg[n_samples + k]; }
    __syncthreads();
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < cap; i += (u64)gridDim.x * blockDim.x) {
        u32 lo = 0, hi = n_samples;  // the last sample whose segment begins at or in front of i (the begins ascend)
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (sbegin[mid] <= i) lo = mid; else hi = mid;
        }
        const u32 s = lo;
        if (i < sbegin[s] || i >= send[s]) continue;
        const u64 key = keys[i];
        const u64 ref = key >> 32;
        if (i > sbegin[s] && (keys[i - 1] >> 32) == ref) continue;
        const u64 cnt = abund_lower_bound(keys + i, send[s] - i, (ref + 1) << 32);
        const u64 up = i + cnt / 2;
        const u32 x1 = (u32)keys[up];
        if (ref < n_refs) med[(u64)s * n_refs + ref] = (cnt & 1) ? (double)x1 : 0.5 * ((double)(u32)keys[up - 1] + (double)x1);
    }
}

// The medians of a sample whose segment does not fit the key buffer (workgroup s; every other workgroup leaves at once).
// Without a place to sort in, the rank of a single-holder hit x among the hits of its reference is COUNTED: the sample is
// walked once per 256 hits, 256 looked-up hashes at a time through LDS, `before` = the hits of x's reference that sort in front
// of x by (abundance, place).  The hit of rank cnt / 2 is the upper median, the largest abundance in front of it the lower
// one.  O(n^2 / 256) per sample: the price of a total_hashes below the offsets' own, not a path a caller should be on.
__global__ void __launch_bounds__(AB_THREADS) k_abund_batch_median_spilled(const AbundBatch q, double* __restrict__ med) {
    __shared__ u32 yref[AB_THREADS], yab[AB_THREADS];
    const u32 s = blockIdx.x;
    const u64 base = q.soff[s], end = q.soff[s + 1];
    if (end <= q.cap || end <= base) return;  // (workgroup-uniform)
    const u64 n = end - base;
    for (u64 x0 = 0; x0 < n; x0 += AB_THREADS) {  // (workgroup-uniform)
        const u64 kx = x0 + threadIdx.x;
        const u32 rx = abund_single_holder(q, base, n, kx);
        const u32 ax = q.abund[base + min(kx, n - 1)];
        u64 cnt = 0, before = 0;
        u32 below = 0;
        for (u64 y0 = 0; y0 < n; y0 += AB_THREADS) {  // (workgroup-uniform)
            __syncthreads();
            yref[threadIdx.x] = abund_single_holder(q, base, n, y0 + threadIdx.x);
            yab[threadIdx.x] = q.abund[base + min(y0 + threadIdx.x, n - 1)];
            __syncthreads();
            if (rx == YH_DIR_NONE) continue;
            const u32 m = (u32)min((u64)AB_THREADS, n - y0);
            for (u32 j = 0; j < m; ++j) {
                if (yref[j] != rx) continue;
                ++cnt;
                if (yab[j] < ax || (yab[j] == ax && y0 + j < kx)) { ++before; below = max(below, yab[j]); }
            }
        }
        if (rx != YH_DIR_NONE && rx < q.n_refs && before == cnt / 2)
            med[(u64)s * q.n_refs + rx] = (cnt & 1) ? (double)ax : 0.5 * ((double)below + (double)ax);
    }
}

}  // namespace

int yh_q_abund(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, u64* d_w_overlap, u64* d_w_match,
               double* d_med_match) {
    hipStream_t st = db->stream;
    const u64 N = db->n_refs;
    if (N == 0) return YH_OK;
    const bool nothing_to_look_up = n_sample == 0 || db->n_distinct == 0;
    // (all-zero bits = 0.0: without a lookup the medians are cleared here too; otherwise k_abund_median writes all of them)
    k_abund_clear<<<(u32)std::min<u64>((N + 255) / 256, 1024), 256, 0, st>>>(
        d_w_overlap, d_w_match, nothing_to_look_up ? reinterpret_cast<u64*>(d_med_match) : nullptr, N);
    if (nothing_to_look_up) {
        YH_HIP(hipGetLastError());
        return YH_OK;
    }
    u64 *d_keys = nullptr, *d_sorted = nullptr, *d_count = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    // the keys sort on the bits that can differ: 32 of abundance and those of a reference id
    unsigned end_bit = 33;
    while (end_bit < 64 && ((N - 1) >> (end_bit - 32)) != 0) ++end_bit;
    int rc = YH_OK;
    do {
        if (d_med_match) {
            if (yh_tmalloc(db, (void**)&d_keys, n_sample * sizeof(u64)) != hipSuccess ||
                yh_tmalloc(db, (void**)&d_sorted, n_sample * sizeof(u64)) != hipSuccess ||
                yh_tmalloc(db, (void**)&d_count, 16) != hipSuccess) { yh_set_error("device allocation failed"); rc = YH_ERR_OOM; break; }
            if (rocprim::radix_sort_keys(nullptr, tmp_bytes, (const u64*)d_keys, d_sorted, (size_t)n_sample, 0u, end_bit, st) != hipSuccess ||
                yh_tmalloc(db, &d_tmp, std::max<size_t>(tmp_bytes, 16)) != hipSuccess) { yh_set_error("device allocation failed"); rc = YH_ERR_OOM; break; }
            // n_hits is known only on the device: all n_sample keys are sorted, the unused tail filled with all ones
            if (hipMemsetAsync(d_keys, 0xff, n_sample * sizeof(u64), st) != hipSuccess ||
                hipMemsetAsync(d_count, 0, 16, st) != hipSuccess) { yh_set_error("hipMemsetAsync failed"); rc = YH_ERR_HIP; break; }
        }
        const YhTileShape shape = yh_tile_shape_for(n_sample);
        const AbundLookup q{d_sample, d_abund, n_sample, yh_dir_view(db), shape.filter ? yh_filter_of(db) : nullptr, db->filter_mul,
                            db->d_po, db->d_pr, d_w_overlap, d_w_match, d_keys, d_count};
        switch (shape.form) {
        case 2: k_abund_lookup<2, 1024, 10><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        case 1: k_abund_lookup<1, 1024, 10><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        default: k_abund_lookup<1, 256, 8><<<shape.tiles(n_sample), 256, 0, st>>>(q); break;
        }
        if (d_med_match) {
            if (rocprim::radix_sort_keys(d_tmp, tmp_bytes, (const u64*)d_keys, d_sorted, (size_t)n_sample, 0u, end_bit, st) != hipSuccess) {
                yh_set_error("radix sort failed: %s", hipGetErrorString(hipGetLastError())); rc = YH_ERR_HIP; break;
            }
            k_abund_median<<<(u32)((N + 255) / 256), 256, 0, st>>>(d_sorted, n_sample, N, d_med_match);
        }
        if (hipGetLastError() != hipSuccess) { yh_set_error("abundance launch failed"); rc = YH_ERR_HIP; }
    } while (0);
    yh_tfree(db, d_tmp); yh_tfree(db, d_keys); yh_tfree(db, d_sorted); yh_tfree(db, d_count);
    return rc;
}

int yh_q_abund_batch(yh_db* db, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples, u64 total_hashes,
                     u64* d_w_overlap, u64* d_w_match, double* d_med_match) {
    hipStream_t st = db->stream;
    const u64 N = db->n_refs;
    if (N == 0) return YH_OK;
    const u64 BN = (u64)n_samples * N;
    const bool looks_up = total_hashes != 0 && db->n_distinct != 0;
    const bool sorts = looks_up && d_med_match;
    const u64 n_tiles = (total_hashes + AB_TILE - 1) / AB_TILE + n_samples;  // (a ragged tile per sample)
    // (the segmented sort counts the keys and reads the segment offsets as 32-bit numbers)
    if (looks_up && ((n_tiles >> 31) || (sorts && (total_hashes >> 32)))) { yh_set_error("batch too large"); return YH_ERR_INVALID_ARG; }
    u64 *d_keys = nullptr, *d_sorted = nullptr;
    u32* d_seg = nullptr;  // [2][n_samples]: the segments' begins, and the ends of their used parts
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    // the keys sort on the bits that can differ: 32 of abundance and those of a reference id
    unsigned end_bit = 33;
    while (end_bit < 64 && ((N - 1) >> (end_bit - 32)) != 0) ++end_bit;
    int rc = YH_OK;
    do {
        if (sorts) {
            if (yh_tmalloc(db, (void**)&d_keys, total_hashes * sizeof(u64)) != hipSuccess ||
                yh_tmalloc(db, (void**)&d_sorted, total_hashes * sizeof(u64)) != hipSuccess ||
                yh_tmalloc(db, (void**)&d_seg, 2 * AB_MAX * sizeof(u32)) != hipSuccess) { yh_set_error("device allocation failed"); rc = YH_ERR_OOM; break; }
            if (rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, (const u64*)d_keys, d_sorted, (unsigned)total_hashes, n_samples,
                                                   (const u32*)d_seg, (const u32*)d_seg + n_samples, 0u, end_bit, st) != hipSuccess ||
                yh_tmalloc(db, &d_tmp, std::max<size_t>(tmp_bytes, 16)) != hipSuccess) { yh_set_error("device allocation failed"); rc = YH_ERR_OOM; break; }
        }
        // every cell of the n_samples rows is written by every call (all-zero bits = 0.0: the median kernels store only the runs that exist)
        k_abund_batch_clear<<<(u32)std::min<u64>((BN + 255) / 256, 2048), 256, 0, st>>>(
            d_w_overlap, d_w_match, reinterpret_cast<u64*>(d_med_match), BN, d_soff, n_samples, total_hashes, d_seg);
        if (!looks_up) break;
        const AbundBatch q{d_samples, d_soff, d_abund, n_samples, yh_dir_view(db), yh_filter_of(db), db->filter_mul, db->d_po, db->d_pr,
                           N, d_w_overlap, d_w_match, d_keys, d_seg ? d_seg + n_samples : nullptr, total_hashes};
        // (k_explain_batch_lookup's grid: workgroups looping over their slots)
        k_abund_batch_lookup<<<(u32)std::min<u64>((n_tiles + 7) / 8 * 8, 32768ull), AB_THREADS, 0, st>>>(q);
        if (sorts) {
            if (rocprim::segmented_radix_sort_keys(d_tmp, tmp_bytes, (const u64*)d_keys, d_sorted, (unsigned)total_hashes, n_samples,
                                                   (const u32*)d_seg, (const u32*)d_seg + n_samples, 0u, end_bit, st) != hipSuccess) {
                yh_set_error("segmented radix sort failed: %s", hipGetErrorString(hipGetLastError())); rc = YH_ERR_HIP; break;
            }
            k_abund_batch_median<<<(u32)std::min<u64>((total_hashes + 255) / 256, 16384), 256, 0, st>>>(d_sorted, d_seg, n_samples,
                                                                                                       total_hashes, N, d_med_match);
            k_abund_batch_median_spilled<<<n_samples, AB_THREADS, 0, st>>>(q, d_med_match);
        }
    } while (0);
    if (rc == YH_OK && hipGetLastError() != hipSuccess) { yh_set_error("abundance batch launch failed"); rc = YH_ERR_HIP; }
    yh_tfree(db, d_tmp); yh_tfree(db, d_keys); yh_tfree(db, d_sorted); yh_tfree(db, d_seg);
    return rc;
}
