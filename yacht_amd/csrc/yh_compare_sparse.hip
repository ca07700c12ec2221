// yh_compare_sparse.hip — the compare pass driven by the hashes that are actually shared (yh_compare_sparse_device,
// yh_compare_routed: include/yacht_hip.h).  The same exact integers as the dense tiles of yh_compare.hip, by another way.
//
// The dense pass merges every pair of samples in full: |A_i| + |B_j| steps a cell, whatever the pair shares.  Samples of
// loosely related environments share a few dozen hashes a pair.  This route groups the entries of a call by hash and
// touches a cell once per hash the pair really shares:
//   k_sp_records   one record per entry: key = the hash, value = the entry's id (A's entries are numbered 0 .. total_a - 1, B's
//                  follow), bit 31 set when the keep test fails.  No hash value is a sentinel: 0 and 2^64 - 1 are hashes.
//   rocPRIM        radix_sort_pairs over bits [0, hash_bits): stable, so a run of equal hashes lists A's entries in sample
//                  order, then B's.  With keep bytes, a scan and k_sp_compact then squeeze the dropped records out of the
//                  sorted arrays, so that no run ever holds one; the count of the kept stays on the device.
//   k_sp_runs      a workgroup takes a chunk of SP_K sorted records.  The record whose predecessor differs -- the
//                  predecessor of a chunk's first record is the last of the chunk before -- heads a run; its thread walks the
//                  run to its end, into the next chunks if need be (a sample is strictly ascending: a run holds one entry per
//                  sample and side, 4 096 at most), so every run comes out once and whole.  Runs that give a pair (two
//                  holders; in the rectangular call one of each side) are listed: the short ones from the front of the
//                  list, the long ones from its back.  The workgroup gathers its runs, its pair count and its longest run
//                  in LDS and meets the other workgroups in five atomics.
//   k_sp_small     runs of up to SP_R entries, flattened: a workgroup takes 256 listed runs, scans their pair counts in
//                  LDS and strides its threads over the pairs of all of them: the lanes of a wave take consecutive pairs
//                  of consecutive runs, none idles on the many two-holder runs.
//   k_sp_large     one workgroup per longer run: (sample, abundance) of its entries staged in LDS, waves take rows, lanes
//                  stride the columns.
//                  A pair adds 1, min(u, v) and u * v to its cell with 64-bit device-scope atomics; the add to dot_lo returns
//                  the old value, and the one add that wraps past 2^64 adds 1 to dot_hi.  Integer sums do not depend on
//                  arrival order: the matrix is exact and two identical calls give identical bytes.  With no abundances on
//                  either side the three sums are equal: only n_shared is counted, k_sp_finish copies it.
//   k_sp_finish    the symmetric call updates cells i < j only: this pass mirrors them and sets the diagonal from the self rows.
//
// yh_compare_routed picks a route per call.  AUTO does not sort everything to find out: it groups only each sample's prefix
// below 2^(hash_bits - YH_COMPARE_SAMPLE_LOG2) -- contiguous, because samples ascend -- with the same records / sort / runs
// code, reads the eight bytes of the pair count back and scales it.
#include "yh_compare.h"

#include <algorithm>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr u32 SP_R = YH_COMPARE_RUN_SMALL;
constexpr u32 SP_K = YH_COMPARE_SPARSE_CHUNK;
constexpr u32 SP_THREADS = 256;
constexpr u32 SP_PER = SP_K / SP_THREADS;                 // records of a chunk a thread looks at
constexpr u32 SP_MAX_RUN = 2 * YH_COMPARE_MAX_SAMPLES;    // one entry per sample and side
constexpr u32 SP_DROPPED = 0x80000000u;                   // (entry ids stay below 2^31)
constexpr u64 SP_MAX_ENTRIES = 1ull << 31;
static_assert(SP_K % SP_THREADS == 0, "a thread takes SP_PER records of a chunk");
static_assert(SP_R >= 2 && SP_R * (SP_R - 1) / 2 * SP_THREADS < (1u << 31), "the pairs of 256 short runs are counted in 32 bits");

// The fitted cost model (profiles/compare_sparse/fit.txt: least squares on the relative errors of a seven-point sweep, no
// constant below zero; nanoseconds on one MI355X): the sparse route costs SP_C0 + SP_C1 * T + SP_C2 * P for T entries and
// P cell updates, the dense route SP_D0 + SP_D1 * D for D merge steps.
constexpr double SP_C0 = 0.0, SP_C1 = 0.0986726, SP_C2 = 0.0862387;
constexpr double SP_D0 = 2.59138e+06, SP_D1 = 0.00334384;

enum { C_N = 0, C_RUNS, C_PAIRS, C_LONGEST, C_SMALL, C_LARGE, C_COUNT = 8 };  // the counters in the work memory

struct SpArgs {
    CmpSide a, b;
    const u64* lim_a;   // per sample the end of the part that takes part, or null: its whole length
    const u64* lim_b;
    const u64* roff_a;  // per sample where its records start, or null: at its offset (B's behind A's total)
    const u64* roff_b;
    u32 keep_and, keep_eq;
    u32 total_a;        // entry ids: A's entry k is k, B's is total_a + k
    u32 n_rec;          // records written
    u32 symmetric, unit, compact;
    u64* key;           // the sorted records (after the compaction, when there is one)
    u32* val;
    u32* flag;
    u32* rank;
    u64* runs;          // run list: short runs from [0], long runs from [runs_cap - 1] downwards
    u64 runs_cap;
    u64* ctr;
    yh_compare_cell* cells;
    u64 ld;
};

__device__ __forceinline__ u32 sp_count(const SpArgs& q) { return q.compact ? (u32)q.ctr[C_N] : q.n_rec; }

// blockIdx.x is the sample, the workgroups of a row of the grid share its entries: its records
__global__ void __launch_bounds__(SP_THREADS) k_sp_records(const SpArgs q, u64* __restrict__ key, u32* __restrict__ val) {
    const bool is_b = blockIdx.x >= q.a.n;
    const CmpSide& sd = is_b ? q.b : q.a;
    const u32 g = is_b ? blockIdx.x - q.a.n : blockIdx.x;
    const u64* lim = is_b ? q.lim_b : q.lim_a;
    const u64* roff = is_b ? q.roff_b : q.roff_a;
    const u64 id0 = is_b ? q.total_a : 0u;
    const u64 lo = sd.off[g], hi = lim ? lim[g] : sd.off[g + 1];
    const u64 r0 = roff ? roff[g] : id0 + lo;
    for (u64 k = lo + blockIdx.y * SP_THREADS + threadIdx.x; k < hi; k += (u64)gridDim.y * SP_THREADS) {
        const bool dropped = sd.keep && ((u32)sd.keep[k] & q.keep_and) != q.keep_eq;
        const u64 r = r0 + (k - lo);
        if (r >= q.n_rec) break;  // (offsets that disagree with the caller's totals: never a write outside)
        key[r] = sd.h[k];
        val[r] = (u32)(id0 + k) | (dropped ? SP_DROPPED : 0u);
    }
}

__global__ void __launch_bounds__(SP_THREADS) k_sp_flag(const u32* __restrict__ val, u32 n, u32* __restrict__ flag) {
    const u32 p = blockIdx.x * SP_THREADS + threadIdx.x;
    if (p <= n) flag[p] = p < n && !(val[p] & SP_DROPPED);
}

__global__ void __launch_bounds__(SP_THREADS) k_sp_compact(const u64* __restrict__ key_s, const u32* __restrict__ val_s, u32 n,
                                                            const u32* __restrict__ flag, const u32* __restrict__ rank,
                                                            u64* __restrict__ key, u32* __restrict__ val, u64* __restrict__ ctr) {
    const u32 p = blockIdx.x * SP_THREADS + threadIdx.x;
    if (p == 0) ctr[C_N] = rank[n];
    if (p < n && flag[p]) key[rank[p]] = key_s[p], val[rank[p]] = val_s[p];
}

// run descriptor: first record, entries, entries of A
__device__ __forceinline__ u64 sp_desc(u32 start, u32 len, u32 ca) { return (u64)start | ((u64)len << 32) | ((u64)ca << 48); }
__device__ __forceinline__ u32 sp_start(u64 d) { return (u32)d; }
__device__ __forceinline__ u32 sp_len(u64 d) { return (u32)(d >> 32) & 0xffffu; }
__device__ __forceinline__ u32 sp_ca(u64 d) { return (u32)(d >> 48); }
__device__ __forceinline__ u32 sp_pairs(const SpArgs& q, u32 len, u32 ca) { return q.symmetric ? len * (len - 1) / 2 : ca * (len - ca); }

__global__ void __launch_bounds__(SP_THREADS) k_sp_runs(const SpArgs q) {
    __shared__ u64 s_runs[SP_K];
    __shared__ u64 s_pairs;
    __shared__ u32 s_small, s_large, s_longest, s_base_small, s_base_large;
    const u32 tid = threadIdx.x, n = sp_count(q);
    const u32 base = blockIdx.x * SP_K;
    if (base >= n) return;
    if (tid == 0) s_pairs = 0, s_small = 0, s_large = 0, s_longest = 0;
    __syncthreads();
    const u64* __restrict__ key = q.key;
    const u32* __restrict__ val = q.val;
#pragma unroll
    for (u32 i = 0; i < SP_PER; ++i) {
        const u32 p = base + i * SP_THREADS + tid;
        if (p >= n) continue;
        const u64 k = key[p];
        if (p != 0 && key[p - 1] == k) continue;  // (not a head: p - 1 may lie in the chunk before)
        u32 e = p + 1, ca = val[p] < q.total_a;
        while (e < n && e - p < SP_MAX_RUN && key[e] == k) ca += val[e] < q.total_a, ++e;  // (may run into the chunks behind)
        const u32 len = e - p, pairs = sp_pairs(q, len, ca);
        if (!pairs) continue;
        if (len <= SP_R) s_runs[atomicAdd(&s_small, 1u)] = sp_desc(p, len, ca);
        else s_runs[SP_K - 1 - atomicAdd(&s_large, 1u)] = sp_desc(p, len, ca);
        atomicAdd(&s_pairs, (u64)pairs);
        atomicMax(&s_longest, len);
    }
    __syncthreads();
    const u32 n_small = s_small, n_large = s_large;
    if (n_small + n_large == 0) return;
    if (tid == 0) {
        s_base_small = (u32)atomicAdd(&q.ctr[C_SMALL], (u64)n_small);
        s_base_large = (u32)atomicAdd(&q.ctr[C_LARGE], (u64)n_large);
        atomicAdd(&q.ctr[C_RUNS], (u64)(n_small + n_large));
        atomicAdd(&q.ctr[C_PAIRS], s_pairs);
        atomicMax(&q.ctr[C_LONGEST], (u64)s_longest);
    }
    __syncthreads();
    for (u32 i = tid; i < n_small; i += SP_THREADS) q.runs[s_base_small + i] = s_runs[i];
    for (u32 i = tid; i < n_large; i += SP_THREADS) q.runs[q.runs_cap - 1 - (s_base_large + i)] = s_runs[SP_K - 1 - i];
}

// the sample and abundance of an entry id
__device__ __forceinline__ void sp_entry(const SpArgs& q, u32 id, u32& smp, u32& ab) {
    const bool is_b = id >= q.total_a;
    const CmpSide& sd = is_b ? q.b : q.a;
    const u64 k = is_b ? id - q.total_a : id;
    u32 lo = 0, hi = sd.n;  // the last sample whose offset is <= k (an empty sample in front of it has the same offset)
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (sd.off[mid] <= k) lo = mid; else hi = mid;
    }
    smp = lo;
    ab = sd.abund ? sd.abund[k] : 1u;
}

__device__ __forceinline__ void sp_update(const SpArgs& q, u32 row, u32 col, u32 u, u32 v) {
    yh_compare_cell* c = q.cells + (u64)row * q.ld + col;
    atomicAdd((u64*)&c->n_shared, 1ull);
    if (q.unit) return;
    atomicAdd((u64*)&c->sum_min, (u64)min(u, v));
    const u64 p = (u64)u * (u64)v;
    const u64 old = atomicAdd((u64*)&c->dot_lo, p);
    if (old + p < old) atomicAdd((u64*)&c->dot_hi, 1ull);  // (this add wrapped)
}

__global__ void __launch_bounds__(SP_THREADS) k_sp_small(const SpArgs q) {
    __shared__ u64 s_desc[SP_THREADS];
    __shared__ u32 s_pre[SP_THREADS + 1];
    __shared__ u32 s_wave[SP_THREADS / 64];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 n_small = (u32)q.ctr[C_SMALL];
    for (u32 g = blockIdx.x; (u64)g * SP_THREADS < n_small; g += gridDim.x) {
        const u32 r = g * SP_THREADS + tid;
        const u64 d = r < n_small ? q.runs[r] : 0ull;
        u32 v = r < n_small ? sp_pairs(q, sp_len(d), sp_ca(d)) : 0u;
        s_desc[tid] = d;
#pragma unroll
        for (u32 s = 1; s < 64; s <<= 1) {
            const u32 t = __shfl_up(v, s);
            if (lane >= s) v += t;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        for (u32 w = 0; w < wave; ++w) v += s_wave[w];
        s_pre[tid + 1] = v;
        if (tid == 0) s_pre[0] = 0;
        __syncthreads();
        const u32 total = s_pre[SP_THREADS];
        for (u32 t = tid; t < total; t += SP_THREADS) {
            u32 lo = 0, hi = SP_THREADS;  // the run this pair belongs to: the last with s_pre <= t
            while (hi - lo > 1) {
                const u32 mid = (lo + hi) >> 1;
                if (s_pre[mid] <= t) lo = mid; else hi = mid;
            }
            const u64 dd = s_desc[lo];
            const u32 start = sp_start(dd), len = sp_len(dd), ca = sp_ca(dd);
            u32 e = t - s_pre[lo], i, j;
            if (q.symmetric) {
                i = 0;
                while (e >= len - 1 - i) e -= len - 1 - i, ++i;  // (row i holds the pairs (i, i + 1 .. len - 1))
                j = i + 1 + e;
            } else {
                const u32 cb = len - ca;
                i = e / cb, j = ca + e % cb;
            }
            u32 si, sj, u, w2;
            sp_entry(q, q.val[start + i], si, u);
            sp_entry(q, q.val[start + j], sj, w2);
            sp_update(q, si, sj, u, w2);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(SP_THREADS) k_sp_large(const SpArgs q) {
    __shared__ u32 s_ab[SP_MAX_RUN];
    __shared__ u16 s_smp[SP_MAX_RUN];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 n_large = (u32)q.ctr[C_LARGE];
    for (u32 r = blockIdx.x; r < n_large; r += gridDim.x) {
        const u64 d = q.runs[q.runs_cap - 1 - r];
        const u32 start = sp_start(d), len = min(sp_len(d), SP_MAX_RUN), ca = min(sp_ca(d), len);
        for (u32 e = tid; e < len; e += SP_THREADS) {
            u32 s, ab;
            sp_entry(q, q.val[start + e], s, ab);
            s_smp[e] = (u16)s, s_ab[e] = ab;
        }
        __syncthreads();
        const u32 rows = q.symmetric ? len - 1 : ca;
        for (u32 i = wave; i < rows; i += SP_THREADS / 64) {
            const u32 si = s_smp[i], u = s_ab[i];
            for (u32 j = (q.symmetric ? i + 1 : ca) + lane; j < len; j += 64) sp_update(q, si, s_smp[j], u, s_ab[j]);
        }
        __syncthreads();
    }
}

// symmetric: the diagonal from the self rows, the lower triangle from the upper; without abundances the two sums that equal n_shared
__global__ void __launch_bounds__(SP_THREADS) k_sp_finish(const SpArgs q, const yh_compare_self* __restrict__ self_a) {
    const u64 t = blockIdx.x * (u64)SP_THREADS + threadIdx.x;
    const u32 n_b = q.symmetric ? q.a.n : q.b.n;
    if (t >= (u64)q.a.n * n_b) return;
    const u32 i = (u32)(t / n_b), j = (u32)(t % n_b);
    yh_compare_cell* c = q.cells + (u64)i * q.ld + j;
    if (q.symmetric && i == j) {
        const yh_compare_self s = self_a[i];
        *c = yh_compare_cell{s.n_kept, s.sum, s.sq_lo, s.sq_hi};
    } else if (q.symmetric && i > j) {
        const yh_compare_cell* m = q.cells + (u64)j * q.ld + i;
        if (q.unit) { const u64 n = m->n_shared; *c = yh_compare_cell{n, n, n, 0}; }  // (the mirror's other words may be written just now)
        else *c = *m;
    } else if (q.unit) {
        c->sum_min = c->n_shared, c->dot_lo = c->n_shared;
    }
}

__global__ void k_sp_info(const SpArgs q, u64 dense_steps, yh_compare_sparse_info* __restrict__ info) {
    yh_compare_sparse_info r{};
    r.n_entries = sp_count(q);
    r.n_shared_hashes = q.ctr[C_RUNS];
    r.n_pair_updates = q.ctr[C_PAIRS];
    r.longest_run = q.ctr[C_LONGEST];
    r.dense_steps = dense_steps;
    r.route = YH_COMPARE_ROUTE_SPARSE;
    *info = r;
}

// the work memory for up to `cap` records
struct SpLayout {
    u64 key, key_s, val, val_s, flag, rank, runs, runs_cap, ctr, tmp, tmp_bytes, total;
};

int sp_layout(u64 cap, SpLayout& w) {
    size_t t1 = 0, t2 = 0;
    if (cap) YH_HIP(rocprim::radix_sort_pairs(nullptr, t1, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)cap, 0u, 64u, (hipStream_t) nullptr));
    YH_HIP(rocprim::exclusive_scan(nullptr, t2, (const u32*)nullptr, (u32*)nullptr, 0u, (size_t)cap + 1, rocprim::plus<u32>(), (hipStream_t) nullptr));
    auto up = [](u64 x) { return (x + 255ull) & ~255ull; };
    u64 at = 0;
    w.ctr = at; at += up(C_COUNT * sizeof(u64));
    w.key = at; at += up(cap * sizeof(u64));
    w.key_s = at; at += up(cap * sizeof(u64));
    w.val = at; at += up(cap * sizeof(u32));
    w.val_s = at; at += up(cap * sizeof(u32));
    w.flag = at; at += up((cap + 1) * sizeof(u32));
    w.rank = at; at += up((cap + 1) * sizeof(u32));
    w.runs_cap = cap / 2 + 1;
    w.runs = at; at += up(w.runs_cap * sizeof(u64));
    w.tmp_bytes = up(std::max<u64>(std::max<u64>(t1, t2), 256));
    w.tmp = at; at += w.tmp_bytes;
    w.total = at + 256;  // (room to align the caller's pointer)
    return YH_OK;
}

u32 sp_blocks(u64 n) { return (u32)((n + SP_THREADS - 1) / SP_THREADS); }

u64 dense_steps_of(u64 n_a, u64 n_b, u64 total_a, u64 total_b, bool sym) {
    return sym ? (n_a + 1) * total_a : n_b * total_a + n_a * total_b;  // (symmetric: the cells i <= j)
}

// records, sort, compaction, runs: leaves the run list and the counters.  q.key / q.val come back pointing at the sorted records.
int sp_group(SpArgs& q, unsigned char* work, const SpLayout& w, u32 hash_bits, hipStream_t st) {
    q.ctr = (u64*)(work + w.ctr);
    q.runs = (u64*)(work + w.runs), q.runs_cap = w.runs_cap;
    q.flag = (u32*)(work + w.flag), q.rank = (u32*)(work + w.rank);
    u64 *key = (u64*)(work + w.key), *key_s = (u64*)(work + w.key_s);
    u32 *val = (u32*)(work + w.val), *val_s = (u32*)(work + w.val_s);
    YH_HIP(hipMemsetAsync(q.ctr, 0, C_COUNT * sizeof(u64), st));
    q.compact = (q.a.keep || q.b.keep) ? 1u : 0u;
    q.key = key_s, q.val = val_s;
    if (!q.n_rec) { q.compact = 0; return YH_OK; }
    const u32 n_smp = q.a.n + (q.symmetric ? 0u : q.b.n);  // (a few long samples still fill the device: 16 entries a thread)
    const u32 per_smp = (u32)std::min<u64>(std::max<u64>((u64)q.n_rec / n_smp / (16 * SP_THREADS), 1), 1024);
    k_sp_records<<<dim3(n_smp, per_smp), SP_THREADS, 0, st>>>(q, key, val);
    size_t tb = w.tmp_bytes;
    YH_HIP(rocprim::radix_sort_pairs(work + w.tmp, tb, (const u64*)key, key_s, (const u32*)val, val_s, (size_t)q.n_rec, 0u, hash_bits, st));
    if (q.compact) {
        k_sp_flag<<<sp_blocks((u64)q.n_rec + 1), SP_THREADS, 0, st>>>(val_s, q.n_rec, q.flag);
        tb = w.tmp_bytes;
        YH_HIP(rocprim::exclusive_scan(work + w.tmp, tb, (const u32*)q.flag, q.rank, 0u, (size_t)q.n_rec + 1, rocprim::plus<u32>(), st));
        k_sp_compact<<<sp_blocks(q.n_rec), SP_THREADS, 0, st>>>(key_s, val_s, q.n_rec, q.flag, q.rank, key, val, q.ctr);
        q.key = key, q.val = val;
    }
    k_sp_runs<<<(u32)(((u64)q.n_rec + SP_K - 1) / SP_K), SP_THREADS, 0, st>>>(q);
    YH_HIP(hipGetLastError());
    return YH_OK;
}

unsigned char* sp_align(void* p) { return reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(p) + 255u) & ~(uintptr_t)255u); }

bool hash_bits_ok(u32 hash_bits) {
    if (hash_bits >= 1 && hash_bits <= 64) return true;
    yh_set_error("hash_bits %u is not in 1 .. 64", hash_bits);
    return false;
}

}  // namespace

extern "C" uint64_t yh_compare_sparse_work_bytes(uint64_t n_a, uint64_t n_b, uint64_t total_a, uint64_t total_b) {
    if (n_a > YH_COMPARE_MAX_SAMPLES || n_b > YH_COMPARE_MAX_SAMPLES || total_a >= SP_MAX_ENTRIES || total_b >= SP_MAX_ENTRIES ||
        total_a + total_b >= SP_MAX_ENTRIES)
        return 0;
    SpLayout w{};
    return sp_layout(total_a + total_b, w) == YH_OK ? w.total : 0;
}

extern "C" int yh_compare_sparse_device(const uint64_t* d_a, const uint64_t* d_a_off, const uint32_t* d_a_abund, const uint8_t* d_a_keep,
                                        uint64_t n_a, uint64_t total_a, const uint64_t* d_b, const uint64_t* d_b_off,
                                        const uint32_t* d_b_abund, const uint8_t* d_b_keep, uint64_t n_b, uint64_t total_b,
                                        uint8_t keep_and, uint8_t keep_eq, yh_compare_cell* d_cells, uint64_t ld_cells,
                                        yh_compare_self* d_self_a, yh_compare_self* d_self_b, void* d_work, uint64_t work_bytes,
                                        void* stream, uint32_t hash_bits, yh_compare_sparse_info* d_info) {
    YH_TRY(compare_args_ok(n_a, n_b, ld_cells));
    if ((n_a && (!d_a_off || !d_self_a)) || (n_b && (!d_b_off || !d_self_b)) || (n_a && n_b && !d_cells) || (total_a && !d_a) ||
        (total_b && !d_b)) {
        yh_set_error("null argument");
        return YH_ERR_INVALID_ARG;
    }
    if (!hash_bits_ok(hash_bits)) return YH_ERR_INVALID_ARG;
    if (total_a >= SP_MAX_ENTRIES || total_b >= SP_MAX_ENTRIES || total_a + total_b >= SP_MAX_ENTRIES) {
        yh_set_error("the sparse compare route takes fewer than 2^31 entries, not %llu + %llu", (u64)total_a, (u64)total_b);
        return YH_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool sym = same_side(d_a, d_a_off, d_a_abund, d_a_keep, n_a, total_a, d_b, d_b_off, d_b_abund, d_b_keep, n_b, total_b);
    if (n_a + n_b == 0) {
        if (d_info) YH_HIP(hipMemsetAsync(d_info, 0, sizeof(*d_info), st));
        return YH_OK;
    }
    SpLayout w{};
    YH_TRY(sp_layout(total_a + total_b, w));
    if (!d_work || work_bytes < w.total) {
        yh_set_error("work buffer holds %llu bytes, %llu needed", (u64)work_bytes, (u64)w.total);
        return YH_ERR_INVALID_ARG;
    }
    unsigned char* work = sp_align(d_work);
    CmpArgs cq{};
    cq.a = CmpSide{(const u64*)d_a, (const u64*)d_a_off, d_a_abund, d_a_keep, (u32)n_a};
    cq.b = CmpSide{(const u64*)d_b, (const u64*)d_b_off, d_b_abund, d_b_keep, (u32)n_b};
    cq.keep_and = keep_and, cq.keep_eq = keep_eq;
    k_compare_self<<<(u32)(n_a + n_b), CMP_THREADS, 0, st>>>(cq, d_self_a, d_self_b);
    if (n_a && n_b)
        YH_HIP(hipMemset2DAsync(d_cells, ld_cells * sizeof(yh_compare_cell), 0, n_b * sizeof(yh_compare_cell), n_a, st));
    SpArgs q{};
    q.a = cq.a, q.b = cq.b;
    q.keep_and = keep_and, q.keep_eq = keep_eq;
    q.total_a = (u32)total_a;
    q.symmetric = sym ? 1u : 0u;
    q.unit = (!d_a_abund && !d_b_abund) ? 1u : 0u;
    q.cells = d_cells, q.ld = ld_cells;
    q.n_rec = (n_a && n_b) ? (u32)(sym ? total_a : total_a + total_b) : 0u;  // (no cells: nothing to group)
    YH_TRY(sp_group(q, work, w, hash_bits, st));
    if (q.n_rec) {
        const u64 groups = ((u64)q.n_rec / 2 + SP_THREADS - 1) / SP_THREADS, longs = (u64)q.n_rec / (SP_R + 1);
        k_sp_small<<<(u32)std::min<u64>(std::max<u64>(groups, 1), 4096), SP_THREADS, 0, st>>>(q);
        if (longs) k_sp_large<<<(u32)std::min<u64>(longs, 2048), SP_THREADS, 0, st>>>(q);
    }
    if (n_a && n_b && (sym || q.unit)) k_sp_finish<<<sp_blocks(n_a * n_b), SP_THREADS, 0, st>>>(q, d_self_a);
    if (d_info) k_sp_info<<<1, 1, 0, st>>>(q, dense_steps_of(n_a, n_b, total_a, total_b, sym), d_info);
    if (hipGetLastError() != hipSuccess) { yh_set_error("sparse compare launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

// the grouping alone -- records, sort, runs -- and its figures: what route auto runs on the samples' prefixes
extern "C" int yh_compare_sparse_count_device(const uint64_t* d_a, const uint64_t* d_a_off, const uint8_t* d_a_keep, uint64_t n_a,
                                              uint64_t total_a, const uint64_t* d_b, const uint64_t* d_b_off, const uint8_t* d_b_keep,
                                              uint64_t n_b, uint64_t total_b, uint8_t keep_and, uint8_t keep_eq, void* d_work,
                                              uint64_t work_bytes, void* stream, uint32_t hash_bits, yh_compare_sparse_info* d_info) {
    YH_TRY(compare_args_ok(n_a, n_b, n_b));
    if ((n_a && !d_a_off) || (n_b && !d_b_off) || (total_a && !d_a) || (total_b && !d_b) || !d_info) {
        yh_set_error("null argument");
        return YH_ERR_INVALID_ARG;
    }
    if (!hash_bits_ok(hash_bits)) return YH_ERR_INVALID_ARG;
    if (total_a >= SP_MAX_ENTRIES || total_b >= SP_MAX_ENTRIES || total_a + total_b >= SP_MAX_ENTRIES) {
        yh_set_error("the sparse compare route takes fewer than 2^31 entries, not %llu + %llu", (u64)total_a, (u64)total_b);
        return YH_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool sym = same_side(d_a, d_a_off, nullptr, d_a_keep, n_a, total_a, d_b, d_b_off, nullptr, d_b_keep, n_b, total_b);
    SpLayout w{};
    YH_TRY(sp_layout(total_a + total_b, w));
    if (!d_work || work_bytes < w.total) {
        yh_set_error("work buffer holds %llu bytes, %llu needed", (u64)work_bytes, (u64)w.total);
        return YH_ERR_INVALID_ARG;
    }
    SpArgs q{};
    q.a = CmpSide{(const u64*)d_a, (const u64*)d_a_off, nullptr, d_a_keep, (u32)n_a};
    q.b = CmpSide{(const u64*)d_b, (const u64*)d_b_off, nullptr, d_b_keep, (u32)n_b};
    q.keep_and = keep_and, q.keep_eq = keep_eq;
    q.total_a = (u32)total_a;
    q.symmetric = sym ? 1u : 0u;
    q.n_rec = (n_a && n_b) ? (u32)(sym ? total_a : total_a + total_b) : 0u;
    YH_TRY(sp_group(q, sp_align(d_work), w, hash_bits, st));
    k_sp_info<<<1, 1, 0, st>>>(q, dense_steps_of(n_a, n_b, total_a, total_b, sym), d_info);
    if (hipGetLastError() != hipSuccess) { yh_set_error("sparse compare launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

namespace {

u32 bits_of_max(const uint64_t* h, const uint64_t* off, u64 n, u32 bits) {
    for (u64 s = 0; s < n; ++s)
        if (off[s + 1] > off[s]) {  // (a sample's last hash is its largest)
            const u64 m = h[off[s + 1] - 1];
            while (bits < 64 && (m >> bits)) ++bits;
        }
    return bits;
}

// the estimator's bounds of one side: per sample the end of its prefix below `window`, and where its records go
void prefix_bounds(const uint64_t* h, const uint64_t* off, u64 n, bool all, u64 window, u64& at, std::vector<u64>& lim, std::vector<u64>& roff) {
    lim.resize(n), roff.resize(n);
    for (u64 s = 0; s < n; ++s) {
        const u64 end = all ? off[s + 1] : (u64)(std::lower_bound(h + off[s], h + off[s + 1], window) - h);
        lim[s] = end, roff[s] = at;
        at += end - off[s];
    }
}

}  // namespace

extern "C" int yh_compare_routed(const uint64_t* a, const uint64_t* a_off, const uint32_t* a_abund, const uint8_t* a_keep, uint64_t n_a,
                                 const uint64_t* b, const uint64_t* b_off, const uint32_t* b_abund, const uint8_t* b_keep, uint64_t n_b,
                                 uint8_t keep_and, uint8_t keep_eq, int device_id, yh_compare_cell* cells, uint64_t ld_cells,
                                 yh_compare_self* self_a, yh_compare_self* self_b, int route, yh_compare_sparse_info* info) {
    if (route != YH_COMPARE_ROUTE_DENSE && route != YH_COMPARE_ROUTE_SPARSE && route != YH_COMPARE_ROUTE_AUTO) {
        yh_set_error("route %d is none of dense (0), sparse (1), auto (2)", route);
        return YH_ERR_INVALID_ARG;
    }
    YH_TRY(compare_args_ok(n_a, n_b, ld_cells));
    if ((n_a && !self_a) || (n_b && !self_b) || (n_a && n_b && !cells)) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    YH_TRY(compare_check_side("A", a, a_off, n_a));
    const bool sym = same_side(a, a_off, a_abund, a_keep, n_a, 0, b, b_off, b_abund, b_keep, n_b, 0);
    if (!sym) YH_TRY(compare_check_side("B", b, b_off, n_b));
    static const uint64_t zero_off[1] = {0};
    if (n_a == 0) a_off = zero_off;
    if (n_b == 0) b_off = zero_off;
    const u64 total_a = a_off[n_a], total_b = b_off[n_b];
    const bool fits = total_a < SP_MAX_ENTRIES && total_b < SP_MAX_ENTRIES && total_a + total_b < SP_MAX_ENTRIES;
    if (route == YH_COMPARE_ROUTE_SPARSE && !fits) {
        yh_set_error("the sparse compare route takes fewer than 2^31 entries, not %llu + %llu", (u64)total_a, (u64)total_b);
        return YH_ERR_INVALID_ARG;
    }
    yh_compare_sparse_info out{};
    out.dense_steps = dense_steps_of(n_a, n_b, total_a, total_b, sym);
    out.route = YH_COMPARE_ROUTE_DENSE;
    if (n_a + n_b == 0) {
        if (info) *info = out;
        return YH_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        yh_set_error("no HIP device available (libyacht_hip has no CPU fallback)");
        return YH_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { yh_set_error("device_id %d out of range", device_id); return YH_ERR_NO_DEVICE; }
    YH_HIP(hipSetDevice(device_id));
    const u32 hash_bits = sym ? bits_of_max(a, a_off, n_a, 1) : bits_of_max(b, b_off, n_b, bits_of_max(a, a_off, n_a, 1));
    CmpDevSide da, db;
    yh_compare_cell* d_cells = nullptr;
    yh_compare_sparse_info* d_info = nullptr;
    u64* d_bounds = nullptr;
    void* d_work = nullptr;
    auto run = [&]() -> int {
        YH_TRY(compare_upload(da, a, a_off, a_abund, a_keep, n_a));
        if (!sym) YH_TRY(compare_upload(db, b, b_off, b_abund, b_keep, n_b));
        const CmpDevSide& rb = sym ? da : db;
        const u64 wb_dense = yh_compare_work_bytes(n_a, n_b, total_a, total_b);
        u64 wb_sparse = 0;
        if (fits && route != YH_COMPARE_ROUTE_DENSE) {
            SpLayout w{};
            YH_TRY(sp_layout(total_a + total_b, w));
            wb_sparse = w.total;
        }
        const u64 wb = std::max(wb_dense, wb_sparse);
        YH_HIP(hipMalloc(&d_work, wb));
        if (n_a && n_b) YH_HIP(hipMalloc((void**)&d_cells, n_a * n_b * sizeof(yh_compare_cell)));
        bool sparse = route == YH_COMPARE_ROUTE_SPARSE;
        if (route == YH_COMPARE_ROUTE_AUTO && fits && n_a && n_b) {
            // the estimator: the pairs among the hashes below the window, by the route's own grouping
            const bool all = hash_bits <= YH_COMPARE_SAMPLE_LOG2;
            const u64 window = all ? 0 : 1ull << (hash_bits - YH_COMPARE_SAMPLE_LOG2);
            std::vector<u64> lim_a, roff_a, lim_b, roff_b;
            u64 n_rec = 0;
            prefix_bounds(a, a_off, n_a, all, window, n_rec, lim_a, roff_a);
            if (!sym) prefix_bounds(b, b_off, n_b, all, window, n_rec, lim_b, roff_b);
            u64 sampled = 0;
            if (n_rec) {
                const u64 n_bounds = 2 * (n_a + (sym ? 0 : n_b));
                std::vector<u64> bounds;
                bounds.reserve(n_bounds);
                bounds.insert(bounds.end(), lim_a.begin(), lim_a.end());
                bounds.insert(bounds.end(), roff_a.begin(), roff_a.end());
                bounds.insert(bounds.end(), lim_b.begin(), lim_b.end());
                bounds.insert(bounds.end(), roff_b.begin(), roff_b.end());
                YH_HIP(hipMalloc((void**)&d_bounds, n_bounds * sizeof(u64)));
                YH_HIP(hipMemcpy(d_bounds, bounds.data(), n_bounds * sizeof(u64), hipMemcpyHostToDevice));
                SpLayout w{};
                YH_TRY(sp_layout(total_a + total_b, w));
                SpArgs q{};
                q.a = CmpSide{(const u64*)da.h, (const u64*)da.off, da.abund, da.keep, (u32)n_a};
                q.b = CmpSide{(const u64*)rb.h, (const u64*)rb.off, rb.abund, rb.keep, (u32)n_b};
                q.lim_a = d_bounds, q.roff_a = d_bounds + n_a;
                if (!sym) q.lim_b = d_bounds + 2 * n_a, q.roff_b = d_bounds + 2 * n_a + n_b;
                q.keep_and = keep_and, q.keep_eq = keep_eq;
                q.total_a = (u32)total_a, q.n_rec = (u32)n_rec, q.symmetric = sym ? 1u : 0u;
                YH_TRY(sp_group(q, sp_align(d_work), w, all ? hash_bits : hash_bits - YH_COMPARE_SAMPLE_LOG2, nullptr));
                YH_HIP(hipMemcpy(&sampled, q.ctr + C_PAIRS, sizeof(u64), hipMemcpyDeviceToHost));  // (the one read-back)
            }
            out.pairs_sampled = sampled;
            out.estimated = all ? 0u : 1u;
            const double p_est = all ? (double)sampled : (double)sampled * (double)(1u << YH_COMPARE_SAMPLE_LOG2);
            const double t_sparse = SP_C0 + SP_C1 * (double)(sym ? total_a : total_a + total_b) + SP_C2 * p_est;
            sparse = t_sparse < SP_D0 + SP_D1 * (double)out.dense_steps;
        }
        if (sparse) {
            if (info) YH_HIP(hipMalloc((void**)&d_info, sizeof(*d_info)));
            YH_TRY(yh_compare_sparse_device(da.h, da.off, da.abund, da.keep, n_a, total_a, rb.h, rb.off, rb.abund, rb.keep, n_b, total_b,
                                            keep_and, keep_eq, d_cells, n_b, da.self, rb.self, d_work, wb, nullptr, hash_bits, d_info));
        } else {
            YH_TRY(yh_compare_device(da.h, da.off, da.abund, da.keep, n_a, total_a, rb.h, rb.off, rb.abund, rb.keep, n_b, total_b, keep_and,
                                     keep_eq, d_cells, n_b, da.self, rb.self, d_work, wb, nullptr));
        }
        YH_HIP(hipDeviceSynchronize());
        if (d_info) {
            yh_compare_sparse_info got{};
            YH_HIP(hipMemcpy(&got, d_info, sizeof(got), hipMemcpyDeviceToHost));
            got.pairs_sampled = out.pairs_sampled, got.estimated = out.estimated;
            out = got;
        } else if (sparse) {
            out.route = YH_COMPARE_ROUTE_SPARSE;
        }
        if (n_a && n_b)
            YH_HIP(hipMemcpy2D(cells, ld_cells * sizeof(yh_compare_cell), d_cells, n_b * sizeof(yh_compare_cell),
                               n_b * sizeof(yh_compare_cell), n_a, hipMemcpyDeviceToHost));
        if (n_a) YH_HIP(hipMemcpy(self_a, da.self, n_a * sizeof(yh_compare_self), hipMemcpyDeviceToHost));
        if (n_b && !(sym && self_b == self_a)) YH_HIP(hipMemcpy(self_b, rb.self, n_b * sizeof(yh_compare_self), hipMemcpyDeviceToHost));
        return YH_OK;
    };
    const int rc = run();
    if (rc != YH_OK) (void)hipDeviceSynchronize();
    da.release();
    db.release();
    (void)hipFree(d_cells);
    (void)hipFree(d_info);
    (void)hipFree(d_bounds);
    (void)hipFree(d_work);
    if (rc == YH_OK && info) *info = out;
    return rc;
}
