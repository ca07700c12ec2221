// yh_lca.hip — every sample hash classified by the LOWEST COMMON ANCESTOR of its holders in a user-supplied taxonomy
// (yh_db_set_taxonomy / yh_lca_device, include/yacht_hip.h).
//
// The taxonomy is a rooted tree over n_nodes nodes (parent[v] < v, depth[v] <= YH_LCA_MAX_DEPTH, node 0 the root) and a leaf
// table leaf[N] that hangs every reference at a node.  For a sample S (strictly ascending) with optional abundances a(h):
//   node[h]      = YH_LCA_NONE when no reference holds h, leaf[j] when j is its only holder, else the LCA of leaf[.] over ALL
//                  of its holders
//   counts[v][0] = number of sample hashes with node[h] == v,  counts[v][1] = sum of a(h) over the same hashes
// The LCA of a shared hash's holders depends on the database and the tree alone: k_lca_index folds it ONCE per taxonomy over the
// shared-hash index into lca_shared[G].  The per-sample pass is then k_explain_lookup's front end -- the directory probe of
// yh_lookup.h, the same tile shapes -- with ONE dependent 4-byte read per hit (leaf[j], or lca_shared[gi]) where the explain
// pass walks a posting list, and k_abund_lookup's LDS hit table keyed by NODE: many shared hits land on few genus or family
// nodes, and the table turns them into one 64-bit atomic per (workgroup, node, column).  Integer adds: the result does not
// depend on arrival order.  parent and depth are 5 bytes per node and stay in the L2.
// A BLOCK of samples takes one clear and one lookup launch (k_lca_batch_lookup, yh_lca_batch_device), and its dense counts
// become rows in (sample, node) order in three more (k_lca_rows_*, yh_lca_rows_pack_device): further down.
#include "yh_lca.h"
#include "yh_lookup.h"

#include <algorithm>
#include <mutex>
#include <unordered_map>

// ---- the handles' taxonomies (yh_lca.h: why they are not members of yh_db) ---------------------------------------------
static std::mutex g_tax_mu;
static std::unordered_map<const yh_db*, YhTaxonomy> g_tax;

YhTaxonomy yh_lca_taxonomy(const yh_db* db) {
    std::lock_guard<std::mutex> lk(g_tax_mu);
    auto it = g_tax.find(db);
    return it == g_tax.end() ? YhTaxonomy{} : it->second;
}

void* yh_lca_taxonomy_swap(const yh_db* db, const YhTaxonomy* t) {
    std::lock_guard<std::mutex> lk(g_tax_mu);
    void* old = nullptr;
    auto it = g_tax.find(db);
    if (it != g_tax.end()) { old = it->second.block; g_tax.erase(it); }
    if (t && t->n_nodes) g_tax[db] = *t;
    return old;
}

namespace {

// One lane per shared hash: the LCA folded along its posting list, holders requested four at a time and their four leaf
// words after them (as or_holders, yh_explain.hip).  The clamped tail re-reads the last holder: harmless, LCA is idempotent.
// A fold that has reached the root leaves the list: nothing can lift it further -- which is what keeps a k-mer that
// thousands of references of many clades share from being one lane's long walk.  (Measured on the 85 205-reference synthetic
// database, 5.3 M shared hashes and 16.1 M postings, longest list 8: 0.25 ms -- profiles/lca/bench_lca.json.  A list of
// thousands of holders INSIDE one clade would be one lane's walk; LCA is associative and commutative, so lists beyond 64
// holders could take a wave each, a strided fold per lane and a shuffle reduction.  Nothing measured asks for it yet.)
__global__ void __launch_bounds__(256) k_lca_index(const u64* __restrict__ po, const u32* __restrict__ pr, u64 n_shared,
                                                   const u32* __restrict__ parent, const u8* __restrict__ depth,
                                                   const u32* __restrict__ leaf, u32* __restrict__ lca_shared) {
    const u64 gi = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (gi >= n_shared) return;
    const u64 q0 = po[gi], qe = po[gi + 1];
    u32 acc = 0;
    if (q0 < qe) {
        acc = leaf[pr[q0]];
        for (u64 q = q0; q < qe && acc != 0; q += 4) {
            u32 h[4], l[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
#pragma unroll
            for (int i = 0; i < 4; ++i) l[i] = leaf[h[i]];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = lca_of(parent, depth, acc, l[i]);
        }
    }
    lca_shared[gi] = acc;
}

struct LcaLookup {
    const u64* sample;
    const u32* abund;  // null: every abundance is 1
    u64 n;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u32* leaf;        // [N]
    const u32* lca_shared;  // [G]
    u32* node;              // [n] or null: counts only
    u64* counts;            // [n_nodes][2], cleared by k_lca_clear before this launch
};

// (tkey: node + 1, 0 = empty; tcnt / tsum: the two columns of that node in this workgroup's tile)
// (51 VGPRs for <2, 1024, 10>, 31 and 30 for the other two shapes, no scratch, 20 KB / 5 KB of LDS: eight waves per SIMD.)
template <int U, int THREADS, int TBITS>
__global__ void __launch_bounds__(THREADS) k_lca_lookup(const LcaLookup q) {
    constexpr u32 TSLOTS = 1u << TBITS;
    __shared__ u32 tkey[TSLOTS];
    __shared__ u64 tcnt[TSLOTS];
    __shared__ u64 tsum[TSLOTS];
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
        ab[u] = abund ? abund[tc] : 1u;
        ok[u] = t < n && h[u] <= dv.max_hash;
        if (!ok[u]) h[u] = 0;  // (still a valid bucket to read)
    }
    for (u32 k = threadIdx.x; k < TSLOTS; k += THREADS) { tkey[k] = 0; tcnt[k] = 0; tsum[k] = 0; }
    YhProbe<U> probe;
    yh_probe_filter<U>(dv, filter, q.filter_mul, h, ok);
    yh_probe_request<U>(dv, h, ok, probe);
    __syncthreads();  // the table is clear
    u32 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = yh_probe_resolve<U>(dv, h, ok, probe, u);
    // the one dependent read of a hit, all of a lane's requested before any is used
    u32 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        v[u] = YH_LCA_NONE;
        if (r[u] != YH_DIR_NONE) v[u] = (r[u] & 0x80000000u) ? q.lca_shared[r[u] & 0x7fffffffu] : q.leaf[r[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const u64 t = base + (u64)u * THREADS + threadIdx.x;
        if (q.node && t < n) q.node[t] = v[u];
        if (v[u] == YH_LCA_NONE) continue;
        const int slot = yh_hit_slot<TBITS>(tkey, v[u]);
        if (slot >= 0) {
            atomicAdd(&tcnt[slot], 1ull);
            if (abund) atomicAdd(&tsum[slot], (u64)ab[u]);
        } else {  // crowded table: sum directly
            atomicAdd(&q.counts[2 * (u64)v[u]], 1ull);
            atomicAdd(&q.counts[2 * (u64)v[u] + 1], (u64)ab[u]);
        }
    }
    __syncthreads();
    for (u32 k = threadIdx.x; k < TSLOTS; k += THREADS)
        if (tkey[k]) {
            const u64 at = 2 * (u64)(tkey[k] - 1);
            atomicAdd(&q.counts[at], tcnt[k]);
            atomicAdd(&q.counts[at + 1], abund ? tsum[k] : tcnt[k]);  // (without abundances the second column is the first)
        }
}

__global__ void __launch_bounds__(256) k_lca_clear(u64* __restrict__ counts, u64 n) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) counts[i] = 0;
}

// ---- the same for a BLOCK of samples under one taxonomy (yh_lca_batch_device) ---------------------------------------------
// A workgroup's unit of work is a tile of LB_TILE consecutive hashes of ONE sample in k_explain_batch_lookup's slot order (the
// resident workgroups share a stretch of the hash range for different samples, and with it the filter and bucket lines), so a
// tile's sample is workgroup-uniform and k_lca_lookup's tail carries over: one dependent 4-byte read per hit, the LDS hit
// table keyed by node -- 2^9 slots for a tile of 1 024 hashes -- flushed once per TILE into counts[s][node] with one 64-bit
// atomic per (tile, node, column) and cleared by the lane that flushed the slot.  A crowded table adds to global memory
// directly.  Integer adds: the result does not depend on arrival order.
// (One hash per lane and round, LB_U = 1: 68 VGPRs, no scratch, 12 304 bytes of LDS -- seven waves per SIMD, the registers
// bound it.  Two per lane took 99 VGPRs, four waves: fewer hashes in flight per SIMD, not more.)
constexpr u32 LB_TILE = YH_LCA_BATCH_TILE;  // (include/yacht_hip.h)
constexpr u32 LB_THREADS = 256;
constexpr int LB_U = 1;
constexpr int LB_TBITS = 9;
constexpr u32 LB_MAX = 256;  // samples per block (include/yacht_hip.h: YH_BATCH_MAX_SAMPLES)
static_assert(LB_TILE % (LB_THREADS * LB_U) == 0, "a tile is whole rounds of the workgroup");

struct LcaBatch {
    const u64* samples;
    const u64* soff;   // [n_samples + 1]
    const u32* abund;  // [total] or null: every abundance is 1
    u32 n_samples;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u32* leaf;        // [N]
    const u32* lca_shared;  // [G]
    u64 n_nodes;
    u32* node;    // [total] or null: counts only
    u64* counts;  // [n_samples][n_nodes][2], cleared in front of this launch
};

__global__ void __launch_bounds__(LB_THREADS) k_lca_batch_lookup(const LcaBatch q) {
    constexpr u32 TSLOTS = 1u << LB_TBITS;
    __shared__ u64 off[LB_MAX + 1];
    __shared__ u64 s_max_nt;
    __shared__ u32 tkey[TSLOTS];
    __shared__ u64 tcnt[TSLOTS];
    __shared__ u64 tsum[TSLOTS];
    const u64* __restrict__ samples = q.samples;
    const u32* __restrict__ abund = q.abund;
    const YhDirView& dv = q.dv;
    const u32* __restrict__ filter = q.filter;
    const u32 n_samples = q.n_samples;
    for (u32 k = threadIdx.x; k <= n_samples; k += LB_THREADS) off[k] = q.soff[k];
    for (u32 k = threadIdx.x; k < TSLOTS; k += LB_THREADS) { tkey[k] = 0; tcnt[k] = 0; tsum[k] = 0; }
    if (threadIdx.x == 0) s_max_nt = 0;
    __syncthreads();
    {   // the longest sample's tiles (one wave: a maximum over <= 256 lengths)
        u64 m = 0;
        if (threadIdx.x < 64)
            for (u32 k = threadIdx.x; k < n_samples; k += 64) m = max(m, (off[k + 1] - off[k] + LB_TILE - 1) / LB_TILE);
        if (threadIdx.x < 64 && m) atomicMax((unsigned long long*)&s_max_nt, (unsigned long long)m);
    }
    __syncthreads();
    const u64 max_nt = uniform64(s_max_nt);
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
        const u64 n_s = uniform64(off[s + 1]) - base, nt_s = (n_s + LB_TILE - 1) / LB_TILE;
        if (nt_s == 0) continue;
        const u64 i = v * nt_s / max_nt;
        if (v > 0 && (v - 1) * nt_s / max_nt == i) continue;  // (a shorter sample: this tile had its slot already)
        u64* __restrict__ counts = q.counts + 2 * (u64)s * q.n_nodes;
        const u64 k_end = min(n_s, (i + 1) * LB_TILE);
        for (u64 k0 = i * LB_TILE; k0 < k_end; k0 += LB_THREADS * LB_U) {  // (workgroup-uniform)
            u64 h[LB_U];
            u32 ab[LB_U];
            bool ok[LB_U];
#pragma unroll
            for (int u = 0; u < LB_U; ++u) {
                const u64 k = k0 + (u64)u * LB_THREADS + threadIdx.x;
                const u64 t = base + min(k, k_end - 1);
                h[u] = samples[t];
                ab[u] = abund ? abund[t] : 1u;
                ok[u] = k < k_end && h[u] <= dv.max_hash;
                if (!ok[u]) h[u] = 0;  // (still a valid word / bucket to read)
            }
            YhProbe<LB_U> probe;
            yh_probe_filter<LB_U>(dv, filter, q.filter_mul, h, ok);
            yh_probe_request<LB_U>(dv, h, ok, probe);
            u32 r[LB_U];
#pragma unroll
            for (int u = 0; u < LB_U; ++u) r[u] = yh_probe_resolve<LB_U>(dv, h, ok, probe, u);
            // the one dependent read of a hit, all of a lane's requested before any is used
            u32 nd[LB_U];
#pragma unroll
            for (int u = 0; u < LB_U; ++u) {
                nd[u] = YH_LCA_NONE;
                if (r[u] != YH_DIR_NONE) nd[u] = (r[u] & 0x80000000u) ? q.lca_shared[r[u] & 0x7fffffffu] : q.leaf[r[u]];
            }
#pragma unroll
            for (int u = 0; u < LB_U; ++u) {
                const u64 k = k0 + (u64)u * LB_THREADS + threadIdx.x;
                if (q.node && k < k_end) q.node[base + k] = nd[u];
                if (nd[u] == YH_LCA_NONE) continue;
                const int slot = yh_hit_slot<LB_TBITS>(tkey, nd[u]);
                if (slot >= 0) {
                    atomicAdd(&tcnt[slot], 1ull);
                    if (abund) atomicAdd(&tsum[slot], (u64)ab[u]);
                } else {  // crowded table: sum directly
                    atomicAdd(&counts[2 * (u64)nd[u]], 1ull);
                    atomicAdd(&counts[2 * (u64)nd[u] + 1], (u64)ab[u]);
                }
            }
        }
        __syncthreads();
        for (u32 k = threadIdx.x; k < TSLOTS; k += LB_THREADS)
            if (tkey[k]) {
                const u64 at = 2 * (u64)(tkey[k] - 1);
                atomicAdd(&counts[at], tcnt[k]);
                atomicAdd(&counts[at + 1], abund ? tsum[k] : tcnt[k]);  // (without abundances the second column is the first)
                tkey[k] = 0; tcnt[k] = 0; tsum[k] = 0;  // (clear for the next slot)
            }
        __syncthreads();
    }
}

// ---- the non-zero cells of a block's dense counts as rows in (sample, node) order (yh_lca_rows_pack_device) ------------------
// Three launches whatever the block: the non-zero cells of every chunk of LP_CHUNK cells counted, the chunk counts scanned by
// ONE workgroup (13 573 chunks for 256 samples x 108 562 nodes: fourteen per lane) into each chunk's first row and the total,
// then every chunk's rows written behind its first: a cell's row is the chunk's first + the non-zero cells of the chunk's
// earlier rounds and waves + those of the lower lanes of its wave (ballots).  No atomic decides a position: the order is the
// cells'.  (6 / 16 / 52 VGPRs, no scratch: eight waves per SIMD; the passes are two reads of the counts' first column.)
constexpr u32 LP_THREADS = 256;
constexpr u32 LP_ROUNDS = 8;
constexpr u32 LP_CHUNK = LP_THREADS * LP_ROUNDS;
constexpr u32 LP_SCAN_THREADS = 1024;

__global__ void __launch_bounds__(LP_THREADS) k_lca_rows_count(const u64* __restrict__ counts, u64 cells, u64* __restrict__ chunk) {
    __shared__ u32 wcnt[LP_THREADS / 64];
    u32 n = 0;
#pragma unroll
    for (u32 r = 0; r < LP_ROUNDS; ++r) {
        const u64 c = blockIdx.x * (u64)LP_CHUNK + r * LP_THREADS + threadIdx.x;
        n += (u32)__popcll(__ballot(c < cells && counts[2 * min(c, cells - 1)] != 0));
    }
    if ((threadIdx.x & 63u) == 0) wcnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 total = 0;
        for (u32 w = 0; w < LP_THREADS / 64; ++w) total += wcnt[w];
        chunk[blockIdx.x] = total;
    }
}

// chunk[b] = the non-zero cells of the chunks before b; *n_rows = all of them.  One workgroup.
__global__ void __launch_bounds__(LP_SCAN_THREADS) k_lca_rows_scan(u64* __restrict__ chunk, u64 n_chunks, u64* __restrict__ n_rows) {
    __shared__ u64 part[LP_SCAN_THREADS];
    const u64 per = (n_chunks + LP_SCAN_THREADS - 1) / LP_SCAN_THREADS;
    const u64 lo = min((u64)threadIdx.x * per, n_chunks), hi = min(lo + per, n_chunks);
    u64 mine = 0;
    for (u64 b = lo; b < hi; ++b) mine += chunk[b];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (u32 d = 1; d < LP_SCAN_THREADS; d <<= 1) {  // (inclusive, in place: read, barrier, add, barrier)
        const u64 below = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += below;
        __syncthreads();
    }
    u64 run = part[threadIdx.x] - mine;
    for (u64 b = lo; b < hi; ++b) {
        const u64 n = chunk[b];
        chunk[b] = run;
        run += n;
    }
    if (threadIdx.x == LP_SCAN_THREADS - 1) *n_rows = part[threadIdx.x];
}

__global__ void __launch_bounds__(LP_THREADS) k_lca_rows_emit(const u64* __restrict__ counts, u64 cells, u64 n_nodes,
                                                              const u64* __restrict__ chunk, yh_lca_row* __restrict__ rows, u64 cap_rows) {
    __shared__ u32 wcnt[LP_ROUNDS * (LP_THREADS / 64)];
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const u64 first = chunk[blockIdx.x];
    if (first >= cap_rows) return;  // (uniform: every row of this chunk lies behind the capacity)
    u64 bal[LP_ROUNDS];
#pragma unroll
    for (u32 r = 0; r < LP_ROUNDS; ++r) {
        const u64 c = blockIdx.x * (u64)LP_CHUNK + r * LP_THREADS + threadIdx.x;
        bal[r] = __ballot(c < cells && counts[2 * min(c, cells - 1)] != 0);
        if (lane == 0) wcnt[r * (LP_THREADS / 64) + wv] = (u32)__popcll(bal[r]);
    }
    __syncthreads();
#pragma unroll
    for (u32 r = 0; r < LP_ROUNDS; ++r) {
        if (!((bal[r] >> lane) & 1ull)) continue;
        u32 below = 0;
        for (u32 w = 0; w < r * (LP_THREADS / 64) + wv; ++w) below += wcnt[w];
        const u64 at = first + below + (u64)__popcll(bal[r] & ((1ull << lane) - 1ull));
        if (at >= cap_rows) continue;
        const u64 c = blockIdx.x * (u64)LP_CHUNK + r * LP_THREADS + threadIdx.x;
        yh_lca_row row;
        row.sample = (u32)(c / n_nodes);
        row.node = (u32)(c % n_nodes);
        row.n_hashes = counts[2 * c];
        row.w_hashes = counts[2 * c + 1];
        rows[at] = row;
    }
}

}  // namespace

int yh_q_lca_index(yh_db* db, const u32* d_parent, const u8* d_depth, const u32* d_leaf, u32* d_lca_shared) {
    const u64 G = db->n_shared;
    if (G == 0) return YH_OK;
    k_lca_index<<<(u32)((G + 255) / 256), 256, 0, db->stream>>>(db->d_po, db->d_pr, G, d_parent, d_depth, d_leaf, d_lca_shared);
    if (hipGetLastError() != hipSuccess) { yh_set_error("lca index launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

int yh_q_lca(yh_db* db, const YhTaxonomy& t, const u64* d_sample, const u32* d_abund, u64 n_sample, u32* d_node, u64* d_counts) {
    hipStream_t st = db->stream;
    const u64 cells = 2 * t.n_nodes;
    k_lca_clear<<<(u32)std::min<u64>((cells + 255) / 256, 1024), 256, 0, st>>>(d_counts, cells);
    if (n_sample != 0 && db->n_refs != 0 && db->n_distinct != 0) {
        const YhTileShape shape = yh_tile_shape_for(n_sample);
        const LcaLookup q{d_sample, d_abund, n_sample, yh_dir_view(db), shape.filter ? yh_filter_of(db) : nullptr, db->filter_mul,
                          t.leaf, t.lca_shared, d_node, d_counts};
        switch (shape.form) {
        case 2: k_lca_lookup<2, 1024, 10><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        case 1: k_lca_lookup<1, 1024, 10><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        default: k_lca_lookup<1, 256, 8><<<shape.tiles(n_sample), 256, 0, st>>>(q); break;
        }
    }
    if (hipGetLastError() != hipSuccess) { yh_set_error("lca launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

int yh_q_lca_batch(yh_db* db, const YhTaxonomy& t, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples,
                   u64 total_hashes, u32* d_node, u64* d_counts) {
    hipStream_t st = db->stream;
    if (hipMemsetAsync(d_counts, 0, 2 * (u64)n_samples * t.n_nodes * sizeof(u64), st) != hipSuccess) { yh_set_error("lca clear failed"); return YH_ERR_HIP; }
    if (total_hashes != 0 && db->n_refs != 0 && db->n_distinct != 0) {
        const u64 n_tiles = (total_hashes + LB_TILE - 1) / LB_TILE + n_samples;  // (a ragged tile per sample)
        const LcaBatch q{d_samples, d_soff, d_abund, n_samples, yh_dir_view(db), yh_filter_of(db), db->filter_mul,
                         t.leaf, t.lca_shared, t.n_nodes, d_node, d_counts};
        // (k_explain_batch_lookup's grid: workgroups looping over their slots)
        k_lca_batch_lookup<<<(u32)std::min<u64>((n_tiles + 7) / 8 * 8, 32768ull), LB_THREADS, 0, st>>>(q);
    }
    if (hipGetLastError() != hipSuccess) { yh_set_error("lca batch launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

int yh_q_lca_rows_pack(yh_db* db, const YhTaxonomy& t, const u64* d_counts, u32 n_samples, yh_lca_row* d_rows, u64 cap_rows,
                       u64* d_n_rows) {
    hipStream_t st = db->stream;
    const u64 cells = (u64)n_samples * t.n_nodes;
    const u64 n_chunks = (cells + LP_CHUNK - 1) / LP_CHUNK;
    u64* d_chunk = nullptr;  // the chunks' counts, then their first rows
    if (yh_tmalloc(db, (void**)&d_chunk, n_chunks * sizeof(u64)) != hipSuccess) { (void)hipGetLastError(); yh_set_error("device allocation failed"); return YH_ERR_OOM; }
    k_lca_rows_count<<<(u32)n_chunks, LP_THREADS, 0, st>>>(d_counts, cells, d_chunk);
    k_lca_rows_scan<<<1, LP_SCAN_THREADS, 0, st>>>(d_chunk, n_chunks, d_n_rows);
    if (cap_rows) k_lca_rows_emit<<<(u32)n_chunks, LP_THREADS, 0, st>>>(d_counts, cells, t.n_nodes, d_chunk, d_rows, cap_rows);
    const bool ok = hipGetLastError() == hipSuccess;
    yh_tfree(db, d_chunk);  // (the cache hands it out again behind this point of the stream)
    if (!ok) { yh_set_error("lca rows pack launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}
