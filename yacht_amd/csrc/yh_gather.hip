// yh_gather.hip — the called references RANKED by the sample hashes each adds (yh_gather_device and, for a block of samples,
// yh_gather_batch_device: include/yacht_hip.h).
//
// For a sample S (strictly ascending), optional abundances a(h) (none: all 1), a candidate table cand[N] and min_hits >= 1:
// a sample hash is LIVE while nobody owns it, c[j] = live sample hashes candidate j holds.  Round k picks the candidate with
// the largest c (ties: the smallest index), stops when c < min_hits, otherwise writes row k = (ref, |S ∩ R_ref|, c, sum of a
// over the live hashes it holds), gives it those hashes, and takes one from the count of every candidate holder of each.
// Holders that are not candidates never count.  It is the one query here in which a reference's result changes every other
// reference's, so it cannot be one pass:
//
//   k_gather_clear    c, solo_n, solo_w, picked [N] and the state words
//   k_gather_lookup   PASS A: the directory probe of yh_lookup.h, once.  A single-holder hit on a candidate r adds to
//                     solo_n[r] / solo_w[r] (through the workgroup's LDS hit table, yh_hit_slot, as the abundance lookup's
//                     sums) and is never looked at again: no other reference can take it, so it is r's when r wins.  A shared
//                     hit with a candidate among its holders adds 1 to c[j] of every candidate holder and appends (sample index, shared index) to the live list (a wave's places by ballot, one returning global
//                     atomic per workgroup; list order is arbitrary and no result depends on it).
//   k_gather_init     c[j] += solo_n[j];  n_overlap[j] = c[j]
//   then per round, and the kernel boundary is the ONLY ordering between workgroups (no workgroup waits on another's word):
//   k_gather_pick     one workgroup: max over the references of (c << 32) | (0xFFFFFFFF - j) -- only a candidate has c > 0;
//                     writes the row with the solo part of w_unique and the winner, or sets `done`; nothing when `done` is set
//   k_gather_claim    grid over the live list; nothing when `done`.  An entry still live whose posting list holds the winner
//                     is marked owned, every candidate holder's c loses one, and its abundance joins the row's w_unique (a
//                     wave sum, one atomic per wave)
//   k_gather_owner    (owner wanted) pass A left the only candidate holder of a single-holder hit in owner[], the claims the
//                     winner of a shared one: what names a reference that was never picked becomes "nobody"
// The host enqueues YH_GATHER_ROUNDS_PER_SYNC rounds (fewer when the cap ends the run sooner), reads `done`, the row count
// and `more` back in one 16-byte copy, and goes on until `done`.  Rounds behind `done` do nothing, so enqueueing past the end
// is harmless.  Integer adds only.
// The single-holder sums with one global atomic per hit took 134 us for a 10^6-hash sample whose 172 000 such hits fall on 294
// candidates (same-address atomics; k_abund_lookup on the same sample: 44 us) and 14.7 us for an 83 k-hash sample with 23 871
// candidates (13.3 us): hence the table (profiles/gather/kernel_stats.txt).
// A BLOCK of samples, each with its own candidates, is ranked by yh_gather_batch_device in the same number of launches as one
// sample -- a pick workgroup per sample, one claim over the live lists of all -- without a host synchronize: the second half
// of this file, under "the same for a BLOCK of samples".
#include "yh_gather.h"
#include "yh_lookup.h"

#include <algorithm>

namespace {

constexpr u32 G_NONE = 0xFFFFFFFFu;   // owner: nobody
constexpr u32 G_OWNED = 0x80000000u;  // a live-list entry's shared index with this bit: taken (shared indices stay below 2^31)
// the state words
enum { G_DONE = 0, G_NROWS = 1, G_MORE = 2, G_WINNER = 3, G_NLIVE = 4, G_WORDS = 8 };

struct GatherLookup {
    const u64* sample;
    const u32* abund;  // null: every abundance is 1
    u64 n;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u64* po;
    const u32* pr;
    const u8* cand;  // [N]
    u32* c;          // [N] the shared part of the counts
    u32* solo_n;     // [N]
    u64* solo_w;     // [N]
    u64* live;       // [n] (sample index << 32) | shared index
    u32* st;         // the state words
    u32* owner;      // [n] or null
};

// c[holder] += 1 for every candidate holder of shared hash gi; the number of candidate holders.  Four holders are requested
// at a time and their four candidate bytes after them (walk_holders / or_holders).
__device__ __forceinline__ u32 count_holders(const u64* __restrict__ po, const u32* __restrict__ pr, const u8* __restrict__ cand,
                                             u32* __restrict__ c, u32 gi) {
    const u64 q0 = po[gi], qe = po[gi + 1];
    u32 n_cand = 0;
    for (u64 q = q0; q < qe; q += 4) {
        u32 h[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = cand[h[i]];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (q + (u64)i < qe && b[i]) { atomicAdd(&c[h[i]], 1u); ++n_cand; }
    }
    return n_cand;
}

// is `ref` among the holders of shared hash gi?  (the clamped tail re-reads the last holder: harmless under OR)
__device__ __forceinline__ bool holds(const u64* __restrict__ po, const u32* __restrict__ pr, u32 gi, u32 ref) {
    const u64 q0 = po[gi], qe = po[gi + 1];
    bool found = false;
    for (u64 q = q0; q < qe; q += 4) {
        u32 h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
        found = found || h[0] == ref || h[1] == ref || h[2] == ref || h[3] == ref;
    }
    return found;
}

// c[holder] -= 1 for every candidate holder of shared hash gi
__device__ __forceinline__ void release_holders(const u64* __restrict__ po, const u32* __restrict__ pr, const u8* __restrict__ cand,
                                                u32* __restrict__ c, u32 gi) {
    const u64 q0 = po[gi], qe = po[gi + 1];
    for (u64 q = q0; q < qe; q += 4) {
        u32 h[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = cand[h[i]];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (q + (u64)i < qe && b[i]) atomicSub(&c[h[i]], 1u);
    }
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (u64)__shfl_xor((unsigned long long)v, d);
    return v;
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (u64)__shfl_xor((unsigned long long)v, d));
    return v;
}

__global__ void __launch_bounds__(256) k_gather_clear(u32* __restrict__ c, u32* __restrict__ solo_n, u64* __restrict__ solo_w,
                                                      u8* __restrict__ picked, u64 n_refs, u32* __restrict__ st) {
    if (blockIdx.x == 0 && threadIdx.x < G_WORDS) st[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 4) c[(n_refs & ~3ull) + threadIdx.x] = 0;  // (the pad k_gather_pick reads)
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < n_refs; j += (u64)gridDim.x * blockDim.x) {
        c[j] = 0;
        solo_n[j] = 0;
        solo_w[j] = 0;
        picked[j] = 0;
    }
}

// (tkey: reference + 1, 0 = empty; tn / tw: the single-holder hits of that candidate in this workgroup's tile and their abundance)
template <int U, int THREADS, int TBITS>
__global__ void __launch_bounds__(THREADS) k_gather_lookup(const GatherLookup q) {
    constexpr u32 TSLOTS = 1u << TBITS;
    __shared__ u32 tkey[TSLOTS];
    __shared__ u32 tn[TSLOTS];
    __shared__ u64 tw[TSLOTS];
    __shared__ u32 wg_live;   // shared hits of this workgroup that go on the live list
    __shared__ u32 wg_first;  // ... and their first place there
    const u64* __restrict__ sample = q.sample;
    const u32* __restrict__ abund = q.abund;
    const u8* __restrict__ cand = q.cand;
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
    for (u32 k = threadIdx.x; k < TSLOTS; k += THREADS) { tkey[k] = 0; tn[k] = 0; tw[k] = 0; }
    if (threadIdx.x == 0) wg_live = 0;
    YhProbe<U> probe;
    yh_probe_filter<U>(dv, filter, q.filter_mul, h, ok);
    yh_probe_request<U>(dv, h, ok, probe);
    __syncthreads();  // the table and wg_live are clear
    const u32 lane = threadIdx.x & 63u;
    u32 place[U], gi[U];
    bool appends[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const u32 r = yh_probe_resolve<U>(dv, h, ok, probe, u);
        u32 own = G_NONE;
        appends[u] = false;
        gi[u] = r & 0x7fffffffu;
        if (r != YH_DIR_NONE) {
            if (r & 0x80000000u) {
                appends[u] = count_holders(q.po, q.pr, cand, q.c, gi[u]) != 0;
            } else if (cand[r]) {
                const int slot = yh_hit_slot<TBITS>(tkey, r);
                if (slot >= 0) {
                    atomicAdd(&tn[slot], 1u);
                    atomicAdd(&tw[slot], (u64)ab[u]);
                } else {  // crowded table: sum directly
                    atomicAdd(&q.solo_n[r], 1u);
                    atomicAdd(&q.solo_w[r], (u64)ab[u]);
                }
                own = r;
            }
        }
        const u64 t = base + (u64)u * THREADS + threadIdx.x;
        if (q.owner && t < n) q.owner[t] = own;
        // the places of the appended hits: a wave's take consecutive ones (a ballot, one returning LDS atomic per wave)
        place[u] = 0;
        const u64 votes = __ballot(appends[u]);
        if (votes) {
            const int leader = __ffsll((long long)votes) - 1;
            u32 first = 0;
            if ((int)lane == leader) first = atomicAdd(&wg_live, (u32)__popcll(votes));
            first = (u32)__shfl((int)first, leader);
            place[u] = first + (u32)__popcll(votes & ((1ull << lane) - 1ull));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_live) wg_first = atomicAdd(&q.st[G_NLIVE], wg_live);
    for (u32 k = threadIdx.x; k < TSLOTS; k += THREADS)
        if (tkey[k]) {
            atomicAdd(&q.solo_n[tkey[k] - 1], tn[k]);
            atomicAdd(&q.solo_w[tkey[k] - 1], tw[k]);
        }
    __syncthreads();
    // (a sample hash appends at most once: at most n entries in all)
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (appends[u]) q.live[(u64)wg_first + place[u]] = ((base + (u64)u * THREADS + threadIdx.x) << 32) | gi[u];
}

__global__ void __launch_bounds__(256) k_gather_init(u32* __restrict__ c, const u32* __restrict__ solo_n, u32* __restrict__ n_overlap,
                                                     u64 n_refs) {
    for (u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x; j < n_refs; j += (u64)gridDim.x * blockDim.x) {
        const u32 v = c[j] + solo_n[j];
        c[j] = v;
        n_overlap[j] = v;
    }
}

constexpr u32 PICK_THREADS = 1024;

// (c is padded to a multiple of four words, the pad zero, and read as 16-byte vectors: a candidate is what has c > 0 -- pass A
// counts candidates only, and min_hits >= 1 -- so the candidate bytes need not be read again)
__global__ void __launch_bounds__(PICK_THREADS) k_gather_pick(u32* c, const u32* __restrict__ n_overlap,
                                                              const u32* __restrict__ solo_n, const u64* __restrict__ solo_w,
                                                              u8* __restrict__ picked, u64 n_refs, u32 min_hits,
                                                              yh_gather_row* __restrict__ rows, u64 cap_rows, u32* __restrict__ st) {
    __shared__ u64 wg_best[PICK_THREADS / 64];
    if (st[G_DONE]) return;  // (uniform: nobody writes the word before the barrier below)
    const uint4* c4 = reinterpret_cast<const uint4*>(c);
    const u64 n4 = (n_refs + 3) / 4;
    u64 best = 0;  // (a reference's key is never 0: its low word is 0xFFFFFFFF - j with j < 2^31)
#pragma unroll 4
    for (u64 v = threadIdx.x; v < n4; v += PICK_THREADS) {
        const uint4 w = c4[v];
        const u32 j = (u32)v * 4u;
        best = max(best, ((u64)w.x << 32) | (u64)(0xFFFFFFFFu - j));
        best = max(best, ((u64)w.y << 32) | (u64)(0xFFFFFFFEu - j));
        best = max(best, ((u64)w.z << 32) | (u64)(0xFFFFFFFDu - j));
        best = max(best, ((u64)w.w << 32) | (u64)(0xFFFFFFFCu - j));
    }
    best = wave_max(best);
    if ((threadIdx.x & 63u) == 0) wg_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (u32 w = 1; w < PICK_THREADS / 64; ++w) best = max(best, wg_best[w]);
    const u32 cnt = (u32)(best >> 32);
    if (cnt < min_hits) {  // (min_hits >= 1: also "no candidate holds a live hash")
        st[G_DONE] = 1;
        return;
    }
    const u32 k = st[G_NROWS];
    if ((u64)k >= cap_rows) {  // stopped at the cap with an eligible candidate left
        st[G_DONE] = 1;
        st[G_MORE] = 1;
        return;
    }
    const u32 j = 0xFFFFFFFFu - (u32)best;
    yh_gather_row row;
    row.ref = j;
    row.n_overlap = n_overlap[j];
    row.n_unique = cnt;
    row.reserved_ = 0;
    row.w_unique = solo_w[j];  // (the shared part: k_gather_claim)
    rows[k] = row;
    picked[j] = 1;
    c[j] = cnt - solo_n[j];  // its single-holder hits are taken here, its live shared ones by the claim
    st[G_WINNER] = j;
    st[G_NROWS] = k + 1;
}

constexpr u32 CLAIM_THREADS = 256;

__global__ void __launch_bounds__(CLAIM_THREADS) k_gather_claim(u64* __restrict__ live, const u32* __restrict__ st,
                                                                const u64* __restrict__ po, const u32* __restrict__ pr,
                                                                const u8* __restrict__ cand, u32* __restrict__ c,
                                                                const u32* __restrict__ abund, yh_gather_row* __restrict__ rows,
                                                                u32* __restrict__ owner) {
    if (st[G_DONE]) return;  // (uniform: no kernel of this launch writes the state words)
    const u64 n_live = st[G_NLIVE];
    const u32 winner = st[G_WINNER];
    unsigned long long* const w_unique = (unsigned long long*)&rows[st[G_NROWS] - 1].w_unique;
    for (u64 i0 = blockIdx.x * (u64)CLAIM_THREADS; i0 < n_live; i0 += (u64)gridDim.x * CLAIM_THREADS) {  // (workgroup-uniform)
        const u64 i = i0 + threadIdx.x;
        bool mine = false;
        u64 a = 0;
        if (i < n_live) {
            const u64 e = live[i];
            const u32 gi = (u32)e;
            if (!(gi & G_OWNED) && holds(po, pr, gi, winner)) {
                release_holders(po, pr, cand, c, gi);
                live[i] = e | G_OWNED;  // (this lane's entry: a plain store)
                const u32 si = (u32)(e >> 32);
                a = abund ? abund[si] : 1u;
                if (owner) owner[si] = winner;
                mine = true;
            }
        }
        if (__ballot(mine) == 0) continue;  // (wave-uniform)
        const u64 sum = wave_sum(a);
        if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(w_unique, (unsigned long long)sum);
    }
}

__global__ void __launch_bounds__(256) k_gather_owner(u32* __restrict__ owner, u64 n, const u8* __restrict__ picked) {
    for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < n; t += (u64)gridDim.x * blockDim.x) {
        const u32 o = owner[t];
        if (o != G_NONE && !picked[o]) owner[t] = G_NONE;
    }
}

__global__ void __launch_bounds__(256) k_gather_nobody(u32* __restrict__ owner, u64 n) {
    for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < n; t += (u64)gridDim.x * blockDim.x) owner[t] = G_NONE;
}

inline u32 grid_for(u64 n, u32 threads, u32 cap) { return (u32)std::min<u64>(std::max<u64>((n + threads - 1) / threads, 1), cap); }

// ---- the same for a BLOCK of samples, each with its own candidates (yh_gather_batch_device) ------------------------------------
// Sample s of the block (laid out as for yh_explain_batch_device) is ranked against the candidates (members[s * N + j] &
// cand_mask) != 0, and every sample's rows, count, `more` and owners are what yh_gather_device gives for it alone.  The single
// call is launch-bound -- a pick and a claim per row, 9.4 us a round with the device almost idle -- so the block pays each
// launch once: every sample has its own c / solo_n / solo_w / n_overlap / picked row (dense [n_samples][N], about 21 bytes a
// cell), its own state words, and its own segment of the live list, live[off[s] .. off[s] + n_live[s]) (a sample hash appends at
// most once, so the segment of a sample is as long as the sample).  A live entry is (position in d_samples << 32) | shared index.
//   k_gather_batch_clear    everything the rounds add to, the state words, d_n_rows and d_more, in 16-byte stores
//   k_gather_batch_lookup   pass A for a tile of GB_TILE consecutive hashes of ONE sample, in k_explain_batch_lookup's tile order:
//                           the same front end, hit table and ballot places as k_gather_lookup; the tile's live entries are
//                           collected in LDS and go to the sample's segment behind one returning atomic per tile
//   k_gather_batch_init     c += solo_n, n_overlap = c, over all cells
//   then per round exactly two launches, whatever n_samples is:
//   k_gather_batch_pick     one workgroup per sample, k_gather_pick on that sample's row; d_n_rows[s] and d_more[s] ARE its row
//                           count and `more` word.  A sample that is done costs one word read; the one that finishes adds 1 to
//                           the block's done count
//   k_gather_batch_claim    leaves when the done count says all are done.  Otherwise every workgroup scans the live tiles
//                           (GB_CLAIM_THREADS entries) of the samples still running into a prefix sum in LDS -- a sample that
//                           is done has none -- and loops over the tiles of the block, finding a tile's sample by a search of
//                           that prefix: the grid is at most GB_CLAIM_GRID workgroups however long the block is
//   k_gather_batch_owner    (owners wanted) as k_gather_owner, a sample per grid row
// The host enqueues min(cap_rows, N) + 1 rounds -- the last pick finds the cap -- and never synchronizes: the outputs are all on
// the device.  cap_rows <= YH_GATHER_BATCH_MAX_ROWS bounds what that enqueues.
constexpr u32 GB_TILE = YH_GATHER_BATCH_TILE;  // (include/yacht_hip.h)
constexpr u32 GB_THREADS = 256;
constexpr u32 GB_TBITS = 9;
constexpr u32 GB_MAX = 256;  // samples per block (include/yacht_hip.h: YH_BATCH_MAX_SAMPLES)
constexpr u32 GB_CLAIM_THREADS = 256;
constexpr u32 GB_CLAIM_GRID = 1024;
static_assert(GB_TILE % GB_THREADS == 0, "a tile is whole rounds of the workgroup");
static_assert(GB_MAX <= GB_CLAIM_THREADS, "the claim scans one sample per thread");
// a sample's state words; the block's done count is the word behind the last sample's
enum { B_DONE = 0, B_WINNER = 1, B_NLIVE = 2, B_WORDS = 4 };

struct GatherBatchLookup {
    const u64* samples;
    const u64* soff;   // [n_samples + 1]
    const u32* abund;  // [total] or null: every abundance is 1
    u32 n_samples;
    YhDirView dv;
    const u32* filter;
    u64 filter_mul;
    const u64* po;
    const u32* pr;
    const u8* members;  // [n_samples][n_refs]
    u32 cand_mask;
    u64 n_refs;
    u32* c;  // [n_samples][c_stride]
    u64 c_stride;
    u32* solo_n;  // [n_samples][n_refs]
    u64* solo_w;  // [n_samples][n_refs]
    u64* live;    // [total]
    u32* st;      // [n_samples][B_WORDS], the done count
    u32* owner;   // [total] or null
};

// count_holders / release_holders with a member row and a mask for the candidate table
__device__ __forceinline__ u32 count_holders_masked(const u64* __restrict__ po, const u32* __restrict__ pr, const u8* __restrict__ member,
                                                    u32 mask, u32* __restrict__ c, u32 gi) {
    const u64 q0 = po[gi], qe = po[gi + 1];
    u32 n_cand = 0;
    for (u64 q = q0; q < qe; q += 4) {
        u32 h[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = member[h[i]] & mask;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (q + (u64)i < qe && b[i]) { atomicAdd(&c[h[i]], 1u); ++n_cand; }
    }
    return n_cand;
}

__device__ __forceinline__ void release_holders_masked(const u64* __restrict__ po, const u32* __restrict__ pr, const u8* __restrict__ member,
                                                       u32 mask, u32* __restrict__ c, u32 gi) {
    const u64 q0 = po[gi], qe = po[gi + 1];
    for (u64 q = q0; q < qe; q += 4) {
        u32 h[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = pr[min(q + (u64)i, qe - 1)];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = member[h[i]] & mask;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (q + (u64)i < qe && b[i]) atomicSub(&c[h[i]], 1u);
    }
}

// (zero: n16 16-byte words; the outputs are cleared by the first workgroup)
__global__ void __launch_bounds__(256) k_gather_batch_clear(uint4* __restrict__ zero, u64 n16, u32* __restrict__ n_rows, u8* __restrict__ more,
                                                            u32 n_samples) {
    if (blockIdx.x == 0)
        for (u32 s = threadIdx.x; s < n_samples; s += blockDim.x) { n_rows[s] = 0; more[s] = 0; }
    for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < n16; k += (u64)gridDim.x * blockDim.x) zero[k] = make_uint4(0, 0, 0, 0);
}

__global__ void __launch_bounds__(GB_THREADS) k_gather_batch_lookup(const GatherBatchLookup q) {
    constexpr u32 TSLOTS = 1u << GB_TBITS;
    __shared__ u64 off[GB_MAX + 1];
    __shared__ u64 s_max_nt;
    __shared__ u32 tkey[TSLOTS];
    __shared__ u32 tn[TSLOTS];
    __shared__ u64 tw[TSLOTS];
    __shared__ u64 ent[GB_TILE];  // this tile's live entries
    __shared__ u32 wg_live;       // ... their number
    __shared__ u32 wg_first;      // ... and their first place in the sample's segment
    const u64* __restrict__ samples = q.samples;
    const u32* __restrict__ abund = q.abund;
    const YhDirView& dv = q.dv;
    const u32* __restrict__ filter = q.filter;
    const u32 n_samples = q.n_samples;
    const u32 mask = q.cand_mask;
    for (u32 k = threadIdx.x; k <= n_samples; k += GB_THREADS) off[k] = q.soff[k];
    if (threadIdx.x == 0) s_max_nt = 0;
    __syncthreads();
    {   // the longest sample's tiles (one wave: a maximum over <= 256 lengths)
        u64 m = 0;
        if (threadIdx.x < 64)
            for (u32 k = threadIdx.x; k < n_samples; k += 64) m = max(m, (off[k + 1] - off[k] + GB_TILE - 1) / GB_TILE);
        if (threadIdx.x < 64 && m) atomicMax((unsigned long long*)&s_max_nt, (unsigned long long)m);
    }
    __syncthreads();
    const u64 max_nt = uniform64(s_max_nt);
    const u32 lane = threadIdx.x & 63u;
    // k_explain_batch_lookup's order: slot (v, s) is tile i = v * nt_s / max_nt of sample s; inside a group of 8 quantile steps x
    // n_samples slots, workgroup l takes step l % 8 of sample l / 8
    const u64 n_slots = max_nt * n_samples;
    const u64 group = 8ull * n_samples;
    for (u64 cs = blockIdx.x; cs < (n_slots + group - 1) / group * group; cs += gridDim.x) {  // (workgroup-uniform)
        const u64 l = cs % group;
        const u64 v = (cs / group) * 8 + (l & 7u);
        const u32 s = (u32)(l >> 3);
        if (v >= max_nt) continue;
        const u64 base = uniform64(off[s]);
        const u64 n_s = uniform64(off[s + 1]) - base, nt_s = (n_s + GB_TILE - 1) / GB_TILE;
        if (nt_s == 0) continue;
        const u64 i = v * nt_s / max_nt;
        if (v > 0 && (v - 1) * nt_s / max_nt == i) continue;  // (a shorter sample: this tile had its slot already)
        for (u32 k = threadIdx.x; k < TSLOTS; k += GB_THREADS) { tkey[k] = 0; tn[k] = 0; tw[k] = 0; }
        if (threadIdx.x == 0) wg_live = 0;
        __syncthreads();
        const u8* __restrict__ member = q.members + (u64)s * q.n_refs;
        u32* __restrict__ c = q.c + (u64)s * q.c_stride;
        u32* __restrict__ solo_n = q.solo_n + (u64)s * q.n_refs;
        u64* __restrict__ solo_w = q.solo_w + (u64)s * q.n_refs;
        const u64 k_end = min(n_s, (i + 1) * GB_TILE);
        for (u64 k0 = i * GB_TILE; k0 < k_end; k0 += GB_THREADS) {  // (workgroup-uniform)
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
            u32 own = G_NONE;
            bool appends = false;
            const u32 gi = r & 0x7fffffffu;
            if (r != YH_DIR_NONE) {
                if (r & 0x80000000u) {
                    appends = count_holders_masked(q.po, q.pr, member, mask, c, gi) != 0;
                } else if (member[r] & mask) {
                    const int slot = yh_hit_slot<GB_TBITS>(tkey, r);
                    if (slot >= 0) {
                        atomicAdd(&tn[slot], 1u);
                        atomicAdd(&tw[slot], (u64)ab);
                    } else {  // crowded table: sum directly
                        atomicAdd(&solo_n[r], 1u);
                        atomicAdd(&solo_w[r], (u64)ab);
                    }
                    own = r;
                }
            }
            if (q.owner && k < k_end) q.owner[base + k] = own;
            // the places of the appended hits: a wave's take consecutive ones (a ballot, one returning LDS atomic per wave)
            const u64 votes = __ballot(appends);
            if (votes) {
                const int leader = __ffsll((long long)votes) - 1;
                u32 first = 0;
                if ((int)lane == leader) first = atomicAdd(&wg_live, (u32)__popcll(votes));
                first = (u32)__shfl((int)first, leader);
                // (only a hit inside the tile appends: at most GB_TILE places)
                if (appends) ent[first + (u32)__popcll(votes & ((1ull << lane) - 1ull))] = ((base + k) << 32) | gi;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0 && wg_live) wg_first = atomicAdd(&q.st[s * B_WORDS + B_NLIVE], wg_live);
        for (u32 k = threadIdx.x; k < TSLOTS; k += GB_THREADS)
            if (tkey[k]) {
                atomicAdd(&solo_n[tkey[k] - 1], tn[k]);
                atomicAdd(&solo_w[tkey[k] - 1], tw[k]);
            }
        __syncthreads();
        // (a sample hash appends at most once: the segment of sample s holds at most n_s entries)
        for (u32 k = threadIdx.x; k < wg_live; k += GB_THREADS) q.live[base + wg_first + k] = ent[k];
        __syncthreads();  // (the table, ent and wg_live are cleared for the next slot)
    }
}

__global__ void __launch_bounds__(256) k_gather_batch_init(u32* __restrict__ c, u64 c_stride, const u32* __restrict__ solo_n,
                                                           u32* __restrict__ n_overlap, u64 n_refs, u32 n_samples) {
    const u64 cells = n_refs * n_samples;
    for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < cells; k += (u64)gridDim.x * blockDim.x) {
        const u64 s = k / n_refs, j = k - s * n_refs;
        const u32 v = c[s * c_stride + j] + solo_n[k];
        c[s * c_stride + j] = v;
        n_overlap[k] = v;
    }
}

// k_gather_pick for sample blockIdx.x: its rows of the tables, its state words, n_rows[s] and more[s]
__global__ void __launch_bounds__(PICK_THREADS) k_gather_batch_pick(u32* c_all, u64 c_stride, const u32* __restrict__ n_overlap_all,
                                                                    const u32* __restrict__ solo_n_all, const u64* __restrict__ solo_w_all,
                                                                    u8* __restrict__ picked_all, u64 n_refs, u32 min_hits,
                                                                    yh_gather_row* __restrict__ rows_all, u64 cap_rows, u32* st_all,
                                                                    u32 n_samples, u32* __restrict__ n_rows, u8* __restrict__ more) {
    __shared__ u64 wg_best[PICK_THREADS / 64];
    const u32 s = blockIdx.x;
    u32* const st = st_all + s * B_WORDS;
    // (uniform: nobody writes the word before the barrier below.  When the whole block is done this sample is: the one read
    // answers both questions)
    if (st[B_DONE]) return;
    u32* const c = c_all + (u64)s * c_stride;
    const uint4* c4 = reinterpret_cast<const uint4*>(c);
    const u64 n4 = (n_refs + 3) / 4;
    u64 best = 0;  // (a reference's key is never 0: its low word is 0xFFFFFFFF - j with j < 2^31)
#pragma unroll 4
    for (u64 v = threadIdx.x; v < n4; v += PICK_THREADS) {
        const uint4 w = c4[v];
        const u32 j = (u32)v * 4u;
        best = max(best, ((u64)w.x << 32) | (u64)(0xFFFFFFFFu - j));
        best = max(best, ((u64)w.y << 32) | (u64)(0xFFFFFFFEu - j));
        best = max(best, ((u64)w.z << 32) | (u64)(0xFFFFFFFDu - j));
        best = max(best, ((u64)w.w << 32) | (u64)(0xFFFFFFFCu - j));
    }
    best = wave_max(best);
    if ((threadIdx.x & 63u) == 0) wg_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (u32 w = 1; w < PICK_THREADS / 64; ++w) best = max(best, wg_best[w]);
    const u32 cnt = (u32)(best >> 32);
    const u32 k = n_rows[s];
    if (cnt < min_hits || (u64)k >= cap_rows) {  // nothing eligible, or stopped at the cap with an eligible candidate left
        if (cnt >= min_hits) more[s] = 1;
        st[B_DONE] = 1;
        atomicAdd(&st_all[n_samples * B_WORDS], 1u);
        return;
    }
    const u32 j = 0xFFFFFFFFu - (u32)best;
    const u64 cell = (u64)s * n_refs + j;
    yh_gather_row row;
    row.ref = j;
    row.n_overlap = n_overlap_all[cell];
    row.n_unique = cnt;
    row.reserved_ = 0;
    row.w_unique = solo_w_all[cell];  // (the shared part: k_gather_batch_claim)
    rows_all[(u64)s * cap_rows + k] = row;
    picked_all[cell] = 1;
    c[j] = cnt - solo_n_all[cell];  // its single-holder hits are taken here, its live shared ones by the claim
    st[B_WINNER] = j;
    n_rows[s] = k + 1;
}

__global__ void __launch_bounds__(GB_CLAIM_THREADS) k_gather_batch_claim(u64* __restrict__ live, const u32* __restrict__ st,
                                                                        u32 n_samples, const u64* __restrict__ soff,
                                                                        const u64* __restrict__ po, const u32* __restrict__ pr,
                                                                        const u8* __restrict__ members, u32 mask, u64 n_refs,
                                                                        u32* __restrict__ c_all, u64 c_stride,
                                                                        const u32* __restrict__ abund, yh_gather_row* __restrict__ rows,
                                                                        u64 cap_rows, const u32* __restrict__ n_rows,
                                                                        u32* __restrict__ owner) {
    __shared__ u32 ends[GB_CLAIM_THREADS];  // live tiles of the samples up to and with this one that still run
    if (st[n_samples * B_WORDS] == n_samples) return;  // (uniform: no kernel of this launch writes the state words)
    u32 n_live = 0;
    if (threadIdx.x < n_samples && !st[threadIdx.x * B_WORDS + B_DONE]) n_live = st[threadIdx.x * B_WORDS + B_NLIVE];
    const u32 my_tiles = (n_live + GB_CLAIM_THREADS - 1) / GB_CLAIM_THREADS;
    ends[threadIdx.x] = my_tiles;
    __syncthreads();
    for (u32 d = 1; d < GB_CLAIM_THREADS; d <<= 1) {
        const u32 add = threadIdx.x >= d ? ends[threadIdx.x - d] : 0;
        __syncthreads();
        ends[threadIdx.x] += add;
        __syncthreads();
    }
    const u32 n_tiles = ends[GB_CLAIM_THREADS - 1];  // (the block holds fewer than 2^32 hashes)
    for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (workgroup-uniform)
        u32 lo = 0, hi = n_samples - 1;  // the first sample whose tiles end behind this one
        while (lo < hi) {
            const u32 mid = (lo + hi) / 2;
            if (ends[mid] > tile) hi = mid; else lo = mid + 1;
        }
        const u32 s = (u32)__builtin_amdgcn_readfirstlane((int)lo);
        const u32 first_tile = s ? ends[s - 1] : 0;
        const u32 len = st[s * B_WORDS + B_NLIVE];
        const u32 winner = st[s * B_WORDS + B_WINNER];
        u64* const seg = live + soff[s];
        const u32 i = (tile - first_tile) * GB_CLAIM_THREADS + threadIdx.x;
        bool mine = false;
        u64 a = 0;
        if (i < len) {
            const u64 e = seg[i];
            const u32 gi = (u32)e;
            if (!(gi & G_OWNED) && holds(po, pr, gi, winner)) {
                release_holders_masked(po, pr, members + (u64)s * n_refs, mask, c_all + (u64)s * c_stride, gi);
                seg[i] = e | G_OWNED;  // (this lane's entry: a plain store)
                const u32 si = (u32)(e >> 32);
                a = abund ? abund[si] : 1u;
                if (owner) owner[si] = winner;
                mine = true;
            }
        }
        if (__ballot(mine) == 0) continue;  // (wave-uniform)
        const u64 sum = wave_sum(a);
        if ((threadIdx.x & 63u) == 0 && sum)
            atomicAdd((unsigned long long*)&rows[(u64)s * cap_rows + n_rows[s] - 1].w_unique, (unsigned long long)sum);
    }
}

// (grid: a row of workgroups per sample)
__global__ void __launch_bounds__(256) k_gather_batch_owner(u32* __restrict__ owner, const u64* __restrict__ soff, const u8* __restrict__ picked,
                                                            u64 n_refs) {
    const u32 s = blockIdx.y;
    const u8* __restrict__ mine = picked + (u64)s * n_refs;
    const u64 end = soff[s + 1];
    for (u64 t = soff[s] + blockIdx.x * (u64)blockDim.x + threadIdx.x; t < end; t += (u64)gridDim.x * blockDim.x) {
        const u32 o = owner[t];
        if (o != G_NONE && !mine[o]) owner[t] = G_NONE;
    }
}

}  // namespace

int yh_q_gather(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, const u8* d_cand, u32 min_hits,
                yh_gather_row* d_rows, u64 cap_rows, u32* d_owner, u64* n_rows, int* more) {
    hipStream_t st = db->stream;
    const u64 N = db->n_refs;
    *n_rows = 0;
    *more = 0;
    if (n_sample == 0 || N == 0 || db->n_distinct == 0) {  // nothing to look up: no row, nobody owns anything
        if (d_owner && n_sample) k_gather_nobody<<<grid_for(n_sample, 256, 2048), 256, 0, st>>>(d_owner, n_sample);
        if (hipGetLastError() != hipSuccess) { yh_set_error("gather launch failed"); return YH_ERR_HIP; }
        return YH_OK;
    }
    u32 *d_c = nullptr, *d_solo_n = nullptr, *d_ovl = nullptr, *d_st = nullptr;
    u64 *d_solo_w = nullptr, *d_live = nullptr;
    u8* d_picked = nullptr;
    int rc = YH_OK;
    do {
        if (yh_tmalloc(db, (void**)&d_c, ((N & ~3ull) + 4) * sizeof(u32)) != hipSuccess || yh_tmalloc(db, (void**)&d_solo_n, N * sizeof(u32)) != hipSuccess ||
            yh_tmalloc(db, (void**)&d_ovl, N * sizeof(u32)) != hipSuccess || yh_tmalloc(db, (void**)&d_solo_w, N * sizeof(u64)) != hipSuccess ||
            yh_tmalloc(db, (void**)&d_picked, N) != hipSuccess || yh_tmalloc(db, (void**)&d_live, n_sample * sizeof(u64)) != hipSuccess ||
            yh_tmalloc(db, (void**)&d_st, G_WORDS * sizeof(u32)) != hipSuccess) { yh_set_error("device allocation failed"); rc = YH_ERR_OOM; break; }
        k_gather_clear<<<grid_for(N, 256, 1024), 256, 0, st>>>(d_c, d_solo_n, d_solo_w, d_picked, N, d_st);
        const YhTileShape shape = yh_tile_shape_for(n_sample);
        const GatherLookup q{d_sample, d_abund, n_sample, yh_dir_view(db), shape.filter ? yh_filter_of(db) : nullptr, db->filter_mul,
                             db->d_po, db->d_pr, d_cand, d_c, d_solo_n, d_solo_w, d_live, d_st, d_owner};
        switch (shape.form) {
        case 2: k_gather_lookup<2, 1024, 10><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        case 1: k_gather_lookup<1, 1024, 10><<<shape.tiles(n_sample), 1024, 0, st>>>(q); break;
        default: k_gather_lookup<1, 256, 8><<<shape.tiles(n_sample), 256, 0, st>>>(q); break;
        }
        k_gather_init<<<grid_for(N, 256, 1024), 256, 0, st>>>(d_c, d_solo_n, d_ovl, N);
        if (hipGetLastError() != hipSuccess) { yh_set_error("gather launch failed"); rc = YH_ERR_HIP; break; }
        // the rounds, a chunk per host sync.  The live list holds at most n_sample entries; its length stays on the device,
        // so the claim's grid is sized by n_sample and its workgroups loop.
        const u32 claim_grid = grid_for(n_sample, CLAIM_THREADS, 1024);
        YhPin pin(4 * sizeof(u32));
        u32 pageable[4] = {0, 0, 0, 0};
        u32* const h_st = pin.p ? (u32*)pin.p : pageable;
        h_st[G_NROWS] = 0;
        for (;;) {
            // (cap_rows - rows so far + 1 rounds end the run whatever the counts are: the last pick finds the cap)
            const u64 rounds = std::min<u64>(YH_GATHER_ROUNDS_PER_SYNC, cap_rows - std::min<u64>(h_st[G_NROWS], cap_rows) + 1);
            for (u64 r = 0; r < rounds; ++r) {
                k_gather_pick<<<1, PICK_THREADS, 0, st>>>(d_c, d_ovl, d_solo_n, d_solo_w, d_picked, N, min_hits, d_rows, cap_rows, d_st);
                k_gather_claim<<<claim_grid, CLAIM_THREADS, 0, st>>>(d_live, d_st, db->d_po, db->d_pr, d_cand, d_c, d_abund, d_rows, d_owner);
            }
            if (hipGetLastError() != hipSuccess) { yh_set_error("gather launch failed"); rc = YH_ERR_HIP; break; }
            if (hipMemcpyAsync(h_st, d_st, 4 * sizeof(u32), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) {
                yh_set_error("gather read-back failed: %s", hipGetErrorString(hipGetLastError()));
                rc = YH_ERR_HIP;
                break;
            }
            if (h_st[G_DONE]) break;
        }
        if (rc != YH_OK) break;
        *n_rows = h_st[G_NROWS];
        *more = (int)h_st[G_MORE];
        if (d_owner) {
            k_gather_owner<<<grid_for(n_sample, 256, 2048), 256, 0, st>>>(d_owner, n_sample, d_picked);
            if (hipGetLastError() != hipSuccess) { yh_set_error("gather launch failed"); rc = YH_ERR_HIP; }
        }
    } while (0);
    yh_tfree(db, d_c); yh_tfree(db, d_solo_n); yh_tfree(db, d_ovl); yh_tfree(db, d_solo_w); yh_tfree(db, d_picked); yh_tfree(db, d_live);
    yh_tfree(db, d_st);
    return rc;
}

int yh_q_gather_batch(yh_db* db, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples, u64 total_hashes,
                      const u8* d_members, u8 cand_mask, u32 min_hits, yh_gather_row* d_rows, u64 cap_rows, u32* d_owner,
                      u32* d_n_rows, u8* d_more) {
    hipStream_t st = db->stream;
    const u64 N = db->n_refs;
    if (total_hashes == 0 || N == 0 || db->n_distinct == 0) {  // nothing to look up: no row, nobody owns anything
        k_gather_batch_clear<<<1, 256, 0, st>>>(nullptr, 0, d_n_rows, d_more, n_samples);
        if (d_owner && total_hashes) k_gather_nobody<<<grid_for(total_hashes, 256, 2048), 256, 0, st>>>(d_owner, total_hashes);
        if (hipGetLastError() != hipSuccess) { yh_set_error("gather batch launch failed"); return YH_ERR_HIP; }
        return YH_OK;
    }
    const u64 n_tiles = (total_hashes + GB_TILE - 1) / GB_TILE + n_samples;  // (a ragged tile per sample)
    if (n_tiles >> 31) { yh_set_error("batch too large"); return YH_ERR_INVALID_ARG; }
    // one block: what the clear zeroes -- c (rows padded to four words and the pad k_gather_batch_pick reads), solo_w, solo_n,
    // the state words, picked -- then n_overlap and the live list, every part at a multiple of 16 bytes
    const u64 B = n_samples, c_stride = (N & ~3ull) + 4;
    auto up16 = [](u64 b) { return (b + 15) & ~15ull; };
    const u64 off_c = 0, off_solo_w = off_c + up16(B * c_stride * sizeof(u32)), off_solo_n = off_solo_w + up16(B * N * sizeof(u64)),
              off_st = off_solo_n + up16(B * N * sizeof(u32)), off_picked = off_st + up16((B * B_WORDS + 1) * sizeof(u32)),
              off_ovl = off_picked + up16(B * N), off_live = off_ovl + up16(B * N * sizeof(u32)),
              bytes = off_live + total_hashes * sizeof(u64);
    u8* d_all = nullptr;
    if (yh_tmalloc(db, (void**)&d_all, bytes) != hipSuccess) { yh_set_error("device allocation failed (%llu bytes for %u samples)", (unsigned long long)bytes, n_samples); return YH_ERR_OOM; }
    u32* const d_c = (u32*)(d_all + off_c);
    u64* const d_solo_w = (u64*)(d_all + off_solo_w);
    u32* const d_solo_n = (u32*)(d_all + off_solo_n);
    u32* const d_st = (u32*)(d_all + off_st);
    u8* const d_picked = d_all + off_picked;
    u32* const d_ovl = (u32*)(d_all + off_ovl);
    u64* const d_live = (u64*)(d_all + off_live);
    k_gather_batch_clear<<<grid_for(off_ovl / 16, 256, 2048), 256, 0, st>>>((uint4*)d_all, off_ovl / 16, d_n_rows, d_more, n_samples);
    const GatherBatchLookup q{d_samples, d_soff, d_abund, n_samples, yh_dir_view(db), yh_filter_of(db), db->filter_mul, db->d_po, db->d_pr,
                              d_members, cand_mask, N, d_c, c_stride, d_solo_n, d_solo_w, d_live, d_st, d_owner};
    // (k_explain_batch_lookup's grid: workgroups looping over their slots)
    k_gather_batch_lookup<<<(u32)std::min<u64>((n_tiles + 7) / 8 * 8, 32768ull), GB_THREADS, 0, st>>>(q);
    k_gather_batch_init<<<grid_for(B * N, 256, 2048), 256, 0, st>>>(d_c, c_stride, d_solo_n, d_ovl, N, n_samples);
    // every round whatever the counts are: a pick that finds its sample done, and a claim that finds the block done, leave at once
    const u32 claim_grid = (u32)std::min<u64>((total_hashes + GB_CLAIM_THREADS - 1) / GB_CLAIM_THREADS + n_samples, GB_CLAIM_GRID);
    const u64 rounds = std::min<u64>(cap_rows, N) + 1;
    for (u64 r = 0; r < rounds; ++r) {
        k_gather_batch_pick<<<n_samples, PICK_THREADS, 0, st>>>(d_c, c_stride, d_ovl, d_solo_n, d_solo_w, d_picked, N, min_hits, d_rows,
                                                               cap_rows, d_st, n_samples, d_n_rows, d_more);
        k_gather_batch_claim<<<claim_grid, GB_CLAIM_THREADS, 0, st>>>(d_live, d_st, n_samples, d_soff, db->d_po, db->d_pr, d_members,
                                                                     cand_mask, N, d_c, c_stride, d_abund, d_rows, cap_rows, d_n_rows,
                                                                     d_owner);
    }
    if (d_owner) {
        const u32 gx = (u32)std::min<u64>(std::max<u64>(total_hashes / n_samples / 256, 1), 256);
        k_gather_batch_owner<<<dim3(gx, n_samples), 256, 0, st>>>(d_owner, d_soff, d_picked, N);
    }
    int rc = YH_OK;
    if (hipGetLastError() != hipSuccess) { yh_set_error("gather batch launch failed"); rc = YH_ERR_HIP; }
    yh_tfree(db, d_all);
    return rc;
}
