// yh_lca.h — the lowest-common-ancestor classification of sample hashes (yh_lca.hip) as yh_api.hip calls it, and the tree walk
// its kernels share with the per-record fold (yh_classify.hip).  Internal, like
// yh_common.h.
#pragma once

#include "yh_common.h"

// The taxonomy of a handle (yh_db_set_taxonomy): one block from the buffer cache and the four arrays inside it.  It is kept
// in a table beside the handles (yh_lca.hip), keyed by the handle, not in yh_db itself: yh_common.h is part of the source the
// PMC traffic files of the run and train kernels are pinned to (profiles/traffic_r06_*.json: source_tag), and a feature that
// touches neither kernel leaves that source, and with it the benchmark's roofline figures, as they are.
struct YhTaxonomy {
    void* block = nullptr;
    const u32* parent = nullptr;      // [n_nodes]
    const u32* leaf = nullptr;        // [N] the node of reference j
    const u32* lca_shared = nullptr;  // [G] the LCA of the leaves of shared hash gi's holders (k_lca_index)
    const u8* depth = nullptr;        // [n_nodes]
    u64 n_nodes = 0, bytes = 0;       // (0 nodes: no taxonomy set)
};
#if defined(__HIPCC__)
// The LCA of nodes a and b: the deeper one lifted to the other's depth, then both lifted until they meet.  Every loop has
// a fixed trip count with a break: the tree has passed the host's validation (depth <= YH_LCA_MAX_DEPTH, parent[v] < v), but
// no input can make this spin.  Two nodes that have not met by then are not in one valid tree: the root.
static __device__ __forceinline__ u32 lca_of(const u32* __restrict__ parent, const u8* __restrict__ depth, u32 a, u32 b) {
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
#endif

// the handle's taxonomy (n_nodes == 0: none set)
YhTaxonomy yh_lca_taxonomy(const yh_db* db);
// Install `t` as the handle's taxonomy (null: remove it).  Returns the block of the one it replaces (or null) for the caller
// to free once nothing reads it any more.  yh_db_destroy removes the entry with the handle.
void* yh_lca_taxonomy_swap(const yh_db* db, const YhTaxonomy* t);

// d_lca_shared[gi] = LCA of d_leaf[holder] over the posting list of shared hash gi, for every gi in [0, db->n_shared), enqueued
// on the handle's stream (yh_db_set_taxonomy).  The tree has passed the host's validation; n_shared == 0 launches nothing.
int yh_q_lca_index(yh_db* db, const u32* d_parent, const u8* d_depth, const u32* d_leaf, u32* d_lca_shared);

// node [n_sample] (d_node may be null: counts only) and counts [n_nodes][2] of one sample against taxonomy `t` of the handle,
// enqueued on the handle's stream (include/yacht_hip.h: yh_lca_device).  d_abund may be null: every abundance is 1.  The
// caller has checked the handle, its taxonomy and the pointers.
int yh_q_lca(yh_db* db, const YhTaxonomy& t, const u64* d_sample, const u32* d_abund, u64 n_sample, u32* d_node, u64* d_counts);

// The same for a block of n_samples samples laid out as for yh_explain_batch_device: node [total_hashes] (may be null) and
// counts [n_samples][n_nodes][2], cleared here, in one clear and one lookup launch (include/yacht_hip.h: yh_lca_batch_device).
// The caller has checked the handle, its taxonomy, the pointers, n_samples and total_hashes.
int yh_q_lca_batch(yh_db* db, const YhTaxonomy& t, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples,
                   u64 total_hashes, u32* d_node, u64* d_counts);

// The non-zero cells of such counts as rows in (sample, node) order, the first cap_rows of them, and their true number in
// *d_n_rows (device): three launches, no host sync (include/yacht_hip.h: yh_lca_rows_pack_device).
int yh_q_lca_rows_pack(yh_db* db, const YhTaxonomy& t, const u64* d_counts, u32 n_samples, yh_lca_row* d_rows, u64 cap_rows,
                       u64* d_n_rows);

// One row per set of the CSR (d_mins, d_off[n_sets + 1]) under taxonomy `t` of the handle, and node [total] (d_node may be null),
// enqueued on the handle's stream: a lookup launch over tiles of entries and a join launch (yh_classify.hip; include/yacht_hip.h:
// yh_classify_sets_device).  The caller has checked the handle, its taxonomy, the pointers, n_sets (1 .. 2^32 - 1) and total.
int yh_q_classify_sets(yh_db* db, const YhTaxonomy& t, const u64* d_mins, const u64* d_off, u64 n_sets, u64 total,
                       yh_classify_row* d_rows, u32* d_node);
