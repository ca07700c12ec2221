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
// caller asks for the median.
#include "yh_abund.h"
#include "yh_lookup.h"

#include <rocprim/device/device_radix_sort.hpp>

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
