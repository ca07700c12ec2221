// yh_classify.hip — a taxon for every RECORD: the sketches of many contigs, bins or reads looked up at once, and the lowest
// common ancestor folded per record on the device (yh_classify_sets_device, include/yacht_hip.h).
// (No reference counterpart; nearest elsewhere: `sourmash lca classify`.)
//
// The input is a CSR of sets as yh_sketch_segments_device leaves it (mins, off[n_sets + 1]): set s owns mins[off[s] ..
// off[s + 1]), strictly ascending inside the set, no order across sets.  node(h) is yh_lca_device's: YH_LCA_NONE, leaf[j] of a
// single holder, or lca_shared[gi].  Per set the call writes ONE row {node, n_kept, n_hit, n_root}: the LCA over the hits that
// are neither NONE nor the root, and the two counts.  16 bytes per record whatever the taxonomy's size -- where the batched
// pass (yh_lca.hip) keeps 16 bytes per (sample, node) cell.
//
// k_classify_lookup: a workgroup takes CL_TILE consecutive ENTRIES, one per lane, and ignores set borders for the probe: the
// three stages of yh_lookup.h and k_lca_lookup's one dependent 4-byte read.  Two lanes find the sets of the tile's first and
// last entry with a clamped search of off (as seg_range, yh_sketch.hip); the offsets between them are staged in LDS when they
// fit, and every entry finds its own set there: the largest s with off[s] <= e, which skips empty sets by itself.  The fold is
// a segmented reduction: shuffle steps 1, 2, .., 32 among lanes of equal set id give every run inside a 64-entry row its LCA
// and its counts; a run that touches neither end of its row is a whole set and writes its row; the rows' first and last
// partials go through LDS to one wave that folds them the same way; what touches neither end of the TILE is a whole set again,
// and the tile's first and last partial become its carry record pair.
// k_classify_join: one lane per carry record; the lane that owns the first record of a set walks the records of that set -- a
// set that spans m tiles is a chain of m joins -- and writes the row.  The same launch writes the rows of the empty sets in a
// grid-stride pass over off, so every row is written by the call and no clear pass runs in front.
// LCA is associative, commutative and idempotent on a validated tree and the counts are integer sums: a row does not depend
// on the tiling or on arrival order.  No atomics, global or LDS.
// (Registers, LDS and scratch as the compiler reports them: profiles/classify/resources.txt.)
#include "yh_lca.h"
#include "yh_lookup.h"

#include <algorithm>

namespace {

constexpr u32 CL_TILE = YH_CLASSIFY_TILE;  // (include/yacht_hip.h)
constexpr u32 CL_THREADS = CL_TILE;        // one entry per lane
constexpr u32 CL_WAVES = CL_THREADS / 64;
constexpr u32 CL_SOFF = 8192;              // offsets of a tile's sets staged in LDS (4 bytes each); beyond: searched in global memory
static_assert(CL_TILE % 64 == 0 && CL_TILE >= 64 && CL_TILE <= 1024, "a tile is whole 64-entry rows of one workgroup");
static_assert(CL_WAVES * 2 <= 64, "one wave folds the rows' partials");

// a partial fold: the set, the LCA of its informative hits so far (YH_LCA_NONE: none yet), hits and root hits
struct ClPart {
    u32 sid, acc, n_hit, n_root;
};

struct ClassifyArgs {
    const u64* mins;
    const u64* off;  // [n_sets + 1]
    u32 n_sets;      // >= 1
    u64 total;       // >= 1, < 2^32
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u32* leaf;        // [N]
    const u32* lca_shared;  // [G]
    const u32* parent;
    const u8* depth;
    yh_classify_row* rows;  // [n_sets]
    u32* node;              // [total] or null
    ClPart* carry;          // [2 * tiles]
};

// the largest s in [lo, hi] with off[s] <= pos (lo when there is none): every read is inside off[lo .. hi], whatever the table
// holds (seg_find, yh_sketch.hip)
__device__ __forceinline__ u32 set_find(const u64* __restrict__ off, u64 pos, u32 lo, u32 hi) {
    while (lo < hi) {
        const u32 m = lo + (hi - lo + 1u) / 2u;
        if (off[m] <= pos) lo = m; else hi = m - 1u;
    }
    return lo;
}

// two partial folds of one set joined.  A fold at the root stays there: nothing can lift it further.
__device__ __forceinline__ u32 fold_join(const u32* __restrict__ parent, const u8* __restrict__ depth, u32 a, u32 b) {
    if (a == YH_LCA_NONE) return b;
    if (b == YH_LCA_NONE) return a;
    if (a == 0u || b == 0u) return 0u;
    return lca_of(parent, depth, a, b);
}

// Inclusive segmented fold along a wave: afterwards the LAST lane of every run of equal sid holds the run's fold and counts
// (cnt: hits in the low half, root hits in the high half -- a tile has at most 1 024 of either).  Set ids ascend along the
// lanes, so an equal id d lanes down means that every lane between belongs to the run as well.
__device__ __forceinline__ void seg_fold(const u32* __restrict__ parent, const u8* __restrict__ depth, u32 lane, u32 sid, u32& acc,
                                         u32& cnt) {
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const u32 s2 = __shfl_up(sid, d, 64);
        const u32 a2 = __shfl_up(acc, d, 64);
        const u32 c2 = __shfl_up(cnt, d, 64);
        if (lane >= d && s2 == sid) {
            acc = fold_join(parent, depth, acc, a2);
            cnt += c2;
        }
    }
}

__device__ __forceinline__ void write_row(const ClassifyArgs& q, u32 sid, u32 acc, u32 n_hit, u32 n_root) {
    yh_classify_row row;
    row.node = acc != YH_LCA_NONE ? acc : (n_hit ? 0u : YH_LCA_NONE);
    row.n_kept = (u32)(q.off[sid + 1] - q.off[sid]);
    row.n_hit = n_hit;
    row.n_root = n_root;
    q.rows[sid] = row;
}

__global__ void __launch_bounds__(CL_THREADS) k_classify_lookup(const ClassifyArgs q) {
    __shared__ u32 lrange[2];
    __shared__ u32 soff[CL_SOFF];
    __shared__ ClPart part[2 * CL_WAVES];
    const YhDirView& dv = q.dv;
    const u64* __restrict__ off = q.off;
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const u64 first = blockIdx.x * (u64)CL_TILE;
    const u64 last = min(first + CL_TILE - 1, q.total - 1);  // (the launch has no workgroup behind the last entry)
    const u64 e = first + threadIdx.x;
    const bool valid = e <= last;
    const u64 ec = min(e, last);
    u64 h[1] = {q.mins[ec]};
    bool ok[1] = {valid && h[0] <= dv.max_hash};
    if (!ok[0]) h[0] = 0;  // (still a valid word / bucket to read)
    if (threadIdx.x == 0) lrange[0] = set_find(off, first, 0u, q.n_sets - 1u);
    if (threadIdx.x == 64 % CL_THREADS) lrange[1] = set_find(off, last, 0u, q.n_sets - 1u);
    YhProbe<1> probe;
    yh_probe_filter<1>(dv, q.filter, q.filter_mul, h, ok);
    yh_probe_request<1>(dv, h, ok, probe);
    __syncthreads();
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)lrange[0]);
    const u32 hi = max(lo, (u32)__builtin_amdgcn_readfirstlane((int)lrange[1]));  // (a bad table: still a range)
    const u32 span = hi - lo;
    const bool staged = span < CL_SOFF;  // (workgroup-uniform)
    if (staged)
        for (u32 k = threadIdx.x; k <= span; k += CL_THREADS) soff[k] = (u32)min(off[lo + k], 0xffffffffull);
    __syncthreads();
    u32 sid;
    if (staged) {  // the same search over the staged offsets (entries lie below 2^32)
        u32 a = 0, b = span;
        const u32 pos = (u32)ec;
        while (a < b) {
            const u32 m = a + (b - a + 1u) / 2u;
            if (soff[m] <= pos) a = m; else b = m - 1u;
        }
        sid = lo + a;
    } else {
        sid = set_find(off, ec, lo, hi);
    }
    const u32 r = yh_probe_resolve<1>(dv, h, ok, probe, 0);
    // the one dependent read of a hit
    u32 v = YH_LCA_NONE;
    if (r != YH_DIR_NONE) v = (r & 0x80000000u) ? q.lca_shared[r & 0x7fffffffu] : q.leaf[r];
    if (q.node && valid) q.node[e] = v;
    // the lanes behind the last entry belong to its set and add nothing
    const bool hit = valid && v != YH_LCA_NONE;
    u32 acc = (hit && v != 0u) ? v : YH_LCA_NONE;
    u32 cnt = (hit ? 1u : 0u) | ((hit && v == 0u) ? 0x10000u : 0u);
    seg_fold(q.parent, q.depth, lane, sid, acc, cnt);
    {
        const u32 s_next = __shfl_down(sid, 1, 64);
        const u32 s0 = __shfl(sid, 0, 64), s63 = __shfl(sid, 63, 64);
        if (lane == 63u || s_next != sid) {  // the last lane of a run
            if (sid == s0) part[2 * wv] = ClPart{sid, acc, cnt & 0xffffu, cnt >> 16};
            else if (sid != s63) write_row(q, sid, acc, cnt & 0xffffu, cnt >> 16);  // touches neither end of the row: a whole set
            if (sid == s63) part[2 * wv + 1] = sid == s0 ? ClPart{sid, YH_LCA_NONE, 0u, 0u} : ClPart{sid, acc, cnt & 0xffffu, cnt >> 16};
        }
    }
    __syncthreads();
    if (wv != 0) return;
    // one wave: the rows' partials, in entry order; the lanes behind them extend the last set and add nothing
    const ClPart p = part[min(lane, 2 * CL_WAVES - 1)];
    const bool mine = lane < 2 * CL_WAVES;
    sid = p.sid;
    acc = mine ? p.acc : YH_LCA_NONE;
    cnt = mine ? (p.n_hit | (p.n_root << 16)) : 0u;
    seg_fold(q.parent, q.depth, lane, sid, acc, cnt);
    const u32 s_next = __shfl_down(sid, 1, 64);
    const u32 s0 = __shfl(sid, 0, 64), s63 = __shfl(sid, 63, 64);
    if (lane == 63u || s_next != sid) {
        ClPart* __restrict__ c = q.carry + 2 * (u64)blockIdx.x;
        if (sid == s0) c[0] = ClPart{sid, acc, cnt & 0xffffu, cnt >> 16};
        else if (sid != s63) write_row(q, sid, acc, cnt & 0xffffu, cnt >> 16);  // touches neither end of the tile: a whole set
        if (sid == s63) c[1] = sid == s0 ? ClPart{sid, YH_LCA_NONE, 0u, 0u} : ClPart{sid, acc, cnt & 0xffffu, cnt >> 16};
    }
}

// The carries joined, and the rows no entry leads to.  n_rec == 0 (nothing was looked up: total == 0 or an empty database):
// every row is {NONE, n_kept, 0, 0} and every node NONE.
__global__ void __launch_bounds__(256) k_classify_join(const ClPart* __restrict__ carry, u64 n_rec, const u64* __restrict__ off, u64 n_sets,
                                                       const u32* __restrict__ parent, const u8* __restrict__ depth,
                                                       yh_classify_row* __restrict__ rows, u32* __restrict__ node, u64 n_node) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    for (u64 i = t0; i < n_rec; i += stride) {
        const ClPart p = carry[i];
        if (i != 0 && carry[i - 1].sid == p.sid) continue;  // (not the set's first record)
        u32 acc = p.acc, n_hit = p.n_hit, n_root = p.n_root;
        for (u64 j = i + 1; j < n_rec; ++j) {
            const ClPart c = carry[j];
            if (c.sid != p.sid) break;
            acc = fold_join(parent, depth, acc, c.acc);
            n_hit += c.n_hit;
            n_root += c.n_root;
        }
        if (p.sid >= n_sets) continue;  // (never: the lookup clamps its set ids)
        yh_classify_row row;
        row.node = acc != YH_LCA_NONE ? acc : (n_hit ? 0u : YH_LCA_NONE);
        row.n_kept = (u32)(off[p.sid + 1] - off[p.sid]);
        row.n_hit = n_hit;
        row.n_root = n_root;
        rows[p.sid] = row;
    }
    for (u64 s = t0; s < n_sets; s += stride) {
        const u64 a = off[s], b = off[s + 1];
        if (n_rec == 0 || a == b) rows[s] = yh_classify_row{YH_LCA_NONE, (u32)(b - a), 0u, 0u};
    }
    if (n_rec == 0 && node)
        for (u64 k = t0; k < n_node; k += stride) node[k] = YH_LCA_NONE;
}

}  // namespace

int yh_q_classify_sets(yh_db* db, const YhTaxonomy& t, const u64* d_mins, const u64* d_off, u64 n_sets, u64 total,
                       yh_classify_row* d_rows, u32* d_node) {
    hipStream_t st = db->stream;
    const bool looks_up = total != 0 && db->n_refs != 0 && db->n_distinct != 0;
    const u64 n_tiles = looks_up ? (total + CL_TILE - 1) / CL_TILE : 0;
    ClPart* d_carry = nullptr;
    if (looks_up) {
        if (yh_tmalloc(db, (void**)&d_carry, 2 * n_tiles * sizeof(ClPart)) != hipSuccess) { (void)hipGetLastError(); yh_set_error("device allocation failed"); return YH_ERR_OOM; }
        const ClassifyArgs q{d_mins, d_off, (u32)n_sets, total, yh_dir_view(db), yh_filter_of(db), db->filter_mul, t.leaf, t.lca_shared,
                             t.parent, t.depth, d_rows, d_node, d_carry};
        k_classify_lookup<<<(u32)n_tiles, CL_THREADS, 0, st>>>(q);
    }
    const u64 lanes = std::max<u64>(std::max<u64>(2 * n_tiles, n_sets), looks_up || !d_node ? 0 : total);
    k_classify_join<<<(u32)std::min<u64>((lanes + 255) / 256, 4096ull), 256, 0, st>>>(d_carry, 2 * n_tiles, d_off, n_sets, t.parent, t.depth,
                                                                                     d_rows, d_node, total);
    const bool ok = hipGetLastError() == hipSuccess;
    yh_tfree(db, d_carry);  // (the cache hands it out again behind this point of the stream)
    if (!ok) { yh_set_error("classify launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}
