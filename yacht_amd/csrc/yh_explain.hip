// yh_explain.hip — what of a sample a set of references explains, PER SAMPLE HASH (yh_explain_device, include/yacht_hip.h).
//
// For a sample S (strictly ascending), optional abundances a(h) (none: all 1) and a member table member[N] whose bit k
// (k in 0..6) says "reference j belongs to call set k":
//   flags[h]     = 0 when no reference of the database holds h, else 0x80 | OR of member[j] over ALL holders j of h
//   totals[b][0] = number of sample hashes whose flag has bit b set,  totals[b][1] = sum of a(h) over the same hashes
// Every other query of the library reduces over the sample and answers [N] arrays; this one answers [n_sample].  It is the
// directory probe of yh_lookup.h again -- the tile shapes, the filter and bucket reads in flight -- with a simpler tail than
// the indexed lookup's: no LDS hit table and no per-reference atomics.  A single-holder hit reads ONE byte of the member table (N bytes: it stays in the L2), a shared hit ORs the bytes of its posting list, and
// each lane stores its own byte (consecutive lanes, consecutive bytes).  The totals are reduced in the wave (a ballot and a
// popcount per bit; a wave sum of the abundances, only for the bits that some lane of the wave has set), then in LDS, and
// leave as at most 16 global atomics per workgroup.  Integer adds and ORs: the result does not depend on arrival order.
#include "yh_explain.h"
#include "yh_lookup.h"

namespace {

struct ExplainLookup {
    const u64* sample;
    const u32* abund;  // null: every abundance is 1
    u64 n;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u64* po;
    const u32* pr;
    const u8* member;  // [N]; bit 7 is masked off here
    u8* flags;         // [n] or null: totals only
    u64* totals;       // [8][2], cleared by k_explain_clear before this launch
};

// OR of the member bytes over the posting list of a shared hash, holders requested four at a time and their four member
// bytes after them (as walk_holders, yh_lookup.h).  The clamped tail re-reads the last holder: harmless under OR.
__device__ __forceinline__ u32 or_holders(const u64* __restrict__ po, const u32* __restrict__ pr, const u8* __restrict__ member, u32 gi) {
    const u64 q0 = po[gi], qe = po[gi + 1];
    u32 m = 0;
    for (u64 q = q0; q < qe; q += 4) {
        u32 h[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = member[h[i]];
        m |= (b[0] | b[1]) | (b[2] | b[3]);
    }
    return m;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (u64)__shfl_xor((unsigned long long)v, d);
    return v;
}

template <int U, int THREADS>
__global__ void __launch_bounds__(THREADS) k_explain_lookup(const ExplainLookup q) {
    __shared__ u64 wg_tot[16];  // this workgroup's [8][2]
    const u64* __restrict__ sample = q.sample;
    const u32* __restrict__ abund = q.abund;
    const u8* __restrict__ member = q.member;
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
        ab[u] = abund ? abund[tc] : 1u;
        ok[u] = t < n && h[u] <= dv.max_hash;
        if (!ok[u]) h[u] = 0;  // (still a valid bucket to read)
    }
    if (threadIdx.x < 16) wg_tot[threadIdx.x] = 0;
    YhProbe<U> probe;
    yh_probe_filter<U>(dv, filter, q.filter_mul, h, ok);
    yh_probe_request<U>(dv, h, ok, probe);
    __syncthreads();  // wg_tot is clear
    u32 f[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const u32 r = yh_probe_resolve<U>(dv, h, ok, probe, u);
        f[u] = 0;
        if (r != YH_DIR_NONE) {
            const u32 m = (r & 0x80000000u) ? or_holders(q.po, q.pr, member, r & 0x7fffffffu) : (u32)member[r];
            f[u] = 0x80u | (m & 0x7fu);
        }
        const u64 t = base + (u64)u * THREADS + threadIdx.x;
        if (q.flags && t < n) q.flags[t] = (u8)f[u];
    }
    // the totals: per bit the wave's count (uniform: a ballot and a popcount) and, for a bit that some lane has set, the
    // wave's abundance sum; lane 0 adds them to the workgroup's 16 words
    const u32 lane = threadIdx.x & 63u;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        u32 cnt = 0;
        u64 mine = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool set = (f[u] >> bit) & 1u;
            cnt += (u32)__popcll(__ballot(set));
            if (set) mine += ab[u];
        }
        if (cnt == 0) continue;  // (uniform)
        const u64 sum = abund ? wave_sum(mine) : (u64)cnt;
        if (lane == 0) {
            atomicAdd(&wg_tot[2 * bit], (u64)cnt);
            atomicAdd(&wg_tot[2 * bit + 1], sum);
        }
    }
    __syncthreads();
    if (threadIdx.x < 16 && wg_tot[threadIdx.x]) atomicAdd(&q.totals[threadIdx.x], wg_tot[threadIdx.x]);
}

__global__ void __launch_bounds__(64) k_explain_clear(u64* __restrict__ totals) {
    if (threadIdx.x < 16) totals[threadIdx.x] = 0;
}

}  // namespace

int yh_q_explain(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, const u8* d_member, u8* d_flags,
                 u64* d_totals) {
    hipStream_t st = db->stream;
    k_explain_clear<<<1, 64, 0, st>>>(d_totals);
    if (n_sample != 0 && db->n_refs != 0 && db->n_distinct != 0) {
        const YhTileShape shape = yh_tile_shape_for(n_sample);
        const ExplainLookup q{d_sample, d_abund, n_sample, yh_dir_view(db), shape.filter ? yh_filter_of(db) : nullptr, db->filter_mul,
                              db->d_po, db->d_pr, d_member, d_flags, d_totals};
        switch (shape.form) {
        case 2: k_explain_lookup<2, 1024><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        case 1: k_explain_lookup<1, 1024><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        default: k_explain_lookup<1, 256><<<shape.tiles(n_sample), 256, 0, st>>>(q); break;
        }
    }
    if (hipGetLastError() != hipSuccess) { yh_set_error("explain launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}
