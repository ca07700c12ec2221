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

// The LCA of nodes a and b: the deeper one lifted to the other's depth, then both lifted until they meet.  Every loop has
// a fixed trip count with a break: the tree has passed the host's validation (depth <= YH_LCA_MAX_DEPTH, parent[v] < v), but
// no input can make this spin.  Two nodes that have not met by then are not in one valid tree: the root.
__device__ __forceinline__ u32 lca_of(const u32* __restrict__ parent, const u8* __restrict__ depth, u32 a, u32 b) {
    if (a == b) return a;
    u32 da = depth[a], db = depth[b];
#pragma unroll 1
    for (int i = 0; i < YH_LCA_MAX_DEPTH; ++i) {
        if (da <= db) break;
        a = parent[a];
        --da;
    }
#pragma unroll 1
    for (int i = 0; i < YH_LCA_MAX_DEPTH; ++i) {
        if (db <= da) break;
        b = parent[b];
        --db;
    }
#pragma unroll 1
    for (int i = 0; i < YH_LCA_MAX_DEPTH; ++i) {
        if (a == b) break;
        a = parent[a];
        b = parent[b];
    }
    return a == b ? a : 0u;
}

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
