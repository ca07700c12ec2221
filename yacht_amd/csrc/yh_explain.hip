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

#include <algorithm>

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

// ---- the same for a BLOCK of samples, each with its own member row (yh_explain_batch_device) --------------------------------
// A workgroup's unit of work is a tile of XB_TILE consecutive hashes of ONE sample, in k_batch_lookup's slot order (yh_batch.hip:
// the workgroups resident at any moment work on the same stretch of the hash range for different samples and share its
// presence-filter lines), so a tile's sample is workgroup-uniform and k_explain_lookup's tail carries over unchanged: per
// round and bit a ballot and a popcount, a wave sum of the abundances for the bits some lane has set, 16 LDS words per
// workgroup, and at most 16 global atomics per tile, into totals[s].  A hit reads members[s * N + ref].  (Keeping the lanes'
// abundance sums in registers over a tile's eight rounds, one wave sum per tile, took 103 VGPRs -- four waves per SIMD; this
// form takes 79, six waves, against k_batch_lookup's 63 and eight.  Forcing eight with a launch bound spills.)
constexpr u32 XB_TILE = YH_EXPLAIN_BATCH_TILE;  // (include/yacht_hip.h)
constexpr u32 XB_THREADS = 256;
constexpr u32 XB_MAX = 256;  // samples per block (include/yacht_hip.h: YH_BATCH_MAX_SAMPLES)
static_assert(XB_TILE % XB_THREADS == 0, "a tile is whole rounds of the workgroup");

struct ExplainBatch {
    const u64* samples;
    const u64* soff;   // [n_samples + 1]
    const u32* abund;  // [total] or null: every abundance is 1
    u32 n_samples;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u64* po;
    const u32* pr;
    const u8* members;  // [n_samples][n_refs]; bit 7 is masked off here
    u64 n_refs;
    u8* flags;    // [total] or null: totals only
    u64* totals;  // [n_samples][8][2], cleared in front of this launch
};

__global__ void __launch_bounds__(XB_THREADS) k_explain_batch_lookup(const ExplainBatch q) {
    __shared__ u64 off[XB_MAX + 1];
    __shared__ u64 s_max_nt;
    __shared__ u64 wg_tot[16];  // this tile's [8][2]
    const u64* __restrict__ samples = q.samples;
    const u32* __restrict__ abund = q.abund;
    const YhDirView& dv = q.dv;
    const u32* __restrict__ filter = q.filter;
    const u32 n_samples = q.n_samples;
    for (u32 k = threadIdx.x; k <= n_samples; k += XB_THREADS) off[k] = q.soff[k];
    if (threadIdx.x == 0) s_max_nt = 0;
    __syncthreads();
    {   // the longest sample's tiles (one wave: a maximum over <= 256 lengths)
        u64 m = 0;
        if (threadIdx.x < 64)
            for (u32 k = threadIdx.x; k < n_samples; k += 64) m = max(m, (off[k + 1] - off[k] + XB_TILE - 1) / XB_TILE);
        if (threadIdx.x < 64 && m) atomicMax((unsigned long long*)&s_max_nt, (unsigned long long)m);
    }
    __syncthreads();
    const u64 max_nt = uniform64(s_max_nt);
    const u32 lane = threadIdx.x & 63u;
    // k_batch_lookup's order: slot (v, s) is tile i = v * nt_s / max_nt of sample s; inside a group of 8 quantile steps x
    // n_samples slots, workgroup l takes step l % 8 of sample l / 8
    const u64 n_slots = max_nt * n_samples;
    const u64 group = 8ull * n_samples;
    for (u64 c = blockIdx.x; c < (n_slots + group - 1) / group * group; c += gridDim.x) {  // (workgroup-uniform)
        const u64 l = c % group;
        const u64 v = (c / group) * 8 + (l & 7u);
        const u32 s = (u32)(l >> 3);
        if (v >= max_nt) continue;
        const u64 base = uniform64(off[s]);
        const u64 n_s = uniform64(off[s + 1]) - base, nt_s = (n_s + XB_TILE - 1) / XB_TILE;
        if (nt_s == 0) continue;
        const u64 i = v * nt_s / max_nt;
        if (v > 0 && (v - 1) * nt_s / max_nt == i) continue;  // (a shorter sample: this tile had its slot already)
        if (threadIdx.x < 16) wg_tot[threadIdx.x] = 0;
        __syncthreads();
        const u8* __restrict__ member = q.members + (u64)s * q.n_refs;
        const u64 k_end = min(n_s, (i + 1) * XB_TILE);
        for (u64 k0 = i * XB_TILE; k0 < k_end; k0 += XB_THREADS) {  // (workgroup-uniform)
            const u64 k = k0 + threadIdx.x;
            const u64 t = base + min(k, k_end - 1);
            u64 h[1] = {samples[t]};
            const u32 ab = abund ? abund[t] : 1u;
            bool ok[1] = {k < k_end && h[0] <= dv.max_hash};
            if (!ok[0]) h[0] = 0;  // (still a valid word / bucket to read)
            YhProbe<1> probe;
            yh_probe_filter<1>(dv, filter, q.filter_mul, h, ok);
            yh_probe_request<1>(dv, h, ok, probe);
            const u32 r = yh_probe_resolve<1>(dv, h, ok, probe, 0);
            u32 f = 0;
            if (r != YH_DIR_NONE) {
                const u32 m = (r & 0x80000000u) ? or_holders(q.po, q.pr, member, r & 0x7fffffffu) : (u32)member[r];
                f = 0x80u | (m & 0x7fu);
            }
            if (q.flags && k < k_end) q.flags[base + k] = (u8)f;
            // k_explain_lookup's tail, once per round: per bit the wave's count and, for a bit some lane has set, its abundance sum
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool set = (f >> bit) & 1u;
                const u32 cnt = (u32)__popcll(__ballot(set));
                if (cnt == 0) continue;  // (uniform)
                const u64 sum = abund ? wave_sum(set ? (u64)ab : 0ull) : (u64)cnt;
                if (lane == 0) {
                    atomicAdd(&wg_tot[2 * bit], (u64)cnt);
                    atomicAdd(&wg_tot[2 * bit + 1], sum);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < 16 && wg_tot[threadIdx.x]) atomicAdd(&q.totals[(u64)s * 16 + threadIdx.x], wg_tot[threadIdx.x]);
        __syncthreads();  // (wg_tot is cleared for the next slot)
    }
}

// members[row.sample][row.ref] = the row's present bytes of up to seven call sets as bits 0..6.  The compact rows name a
// (sample, reference) pair at most once: each row owns its byte (a plain store).  d_members is cleared in front.
__global__ void __launch_bounds__(256) k_explain_members_rows(const yh_batch_row* __restrict__ rows, const u32* __restrict__ n_rows,
                                                              u64 cap_rows, const u8* __restrict__ present, u32 n_sets,
                                                              u32 n_samples, u64 n_refs, u8* __restrict__ members) {
    const u64 n = min((u64)*n_rows, cap_rows);
    for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < n; k += (u64)gridDim.x * blockDim.x) {
        const u32 smp = rows[k].sample, ref = rows[k].ref;
        if (smp >= n_samples || ref >= n_refs) continue;
        u32 m = 0;
#pragma unroll
        for (u32 c = 0; c < 7; ++c)
            if (c < n_sets) m |= (u32)(present[(u64)c * cap_rows + k] != 0) << c;
        members[(u64)smp * n_refs + ref] = (u8)m;
    }
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

int yh_q_explain_batch(yh_db* db, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples, u64 total_hashes,
                       const u8* d_members, u8* d_flags, u64* d_totals) {
    hipStream_t st = db->stream;
    if (hipMemsetAsync(d_totals, 0, (u64)n_samples * 16 * sizeof(u64), st) != hipSuccess) { yh_set_error("explain clear failed"); return YH_ERR_HIP; }
    if (total_hashes != 0 && db->n_refs != 0 && db->n_distinct != 0) {
        const u64 n_tiles = (total_hashes + XB_TILE - 1) / XB_TILE + n_samples;  // (a ragged tile per sample)
        if (n_tiles >> 31) { yh_set_error("batch too large"); return YH_ERR_INVALID_ARG; }
        const ExplainBatch q{d_samples, d_soff, d_abund, n_samples, yh_dir_view(db), yh_filter_of(db), db->filter_mul,
                             db->d_po, db->d_pr, d_members, db->n_refs, d_flags, d_totals};
        // (k_batch_lookup's grid: workgroups looping over their slots, capped where its sweep found the best time)
        k_explain_batch_lookup<<<(u32)std::min<u64>((n_tiles + 7) / 8 * 8, 32768ull), XB_THREADS, 0, st>>>(q);
    }
    if (hipGetLastError() != hipSuccess) { yh_set_error("explain batch launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

int yh_q_explain_members_rows(yh_db* db, const yh_batch_row* d_rows, const u32* d_n_rows, u64 cap_rows, const u8* d_present,
                              u32 n_sets, u32 n_samples, u8* d_members) {
    hipStream_t st = db->stream;
    const u64 N = db->n_refs;
    if (N == 0) return YH_OK;
    if (hipMemsetAsync(d_members, 0, (u64)n_samples * N, st) != hipSuccess) { yh_set_error("member clear failed"); return YH_ERR_HIP; }
    if (cap_rows) {
        const u32 grid = (u32)std::min<u64>((cap_rows + 255) / 256, 4096);
        k_explain_members_rows<<<grid, 256, 0, st>>>(d_rows, d_n_rows, cap_rows, d_present, n_sets, n_samples, N, d_members);
    }
    if (hipGetLastError() != hipSuccess) { yh_set_error("member rows launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}
