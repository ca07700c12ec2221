// yh_gather.hip — the called references RANKED by the sample hashes each adds (yh_gather_device, include/yacht_hip.h).
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
