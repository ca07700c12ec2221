// yh_sketch.hip — DNA FracMinHash sketching on the device.
//
// Replaces the `sourmash sketch dna -p k=K,scaled=S,abund` subprocess of the reference
// (src/yacht/sketch_ref_genomes.py:25,61, sketch_sample.py:32,49) for the hashing part: every
// length-K window made only of A/C/G/T (either case) -> canonical form (lexicographic minimum of
// the k-mer and its reverse complement) -> first 64 bits of MurmurHash3_x64_128 (public domain
// algorithm by Austin Appleby) of its upper-case ASCII bytes, seed 42 -> kept iff <= max_hash.
// One lane per window; the kept hashes (about 1/scaled of the windows) are appended unsorted, with
// duplicates; the caller sorts and counts them (abundances).  ALU-bound, integer only.
//
// The SEGMENTED form (yh_sketch_segments*, further down): the buffer holds many records, seg_off[n_seg + 1] cuts it into
// segments, and one hashing pass yields one finished sketch per segment in HBM.  The same kernels, instantiated with
// SEG = true, emit (segment, hash) pairs: a window belongs to the segment its first byte lies in and counts only when all
// its k bytes lie inside that segment (segments may touch without a separator byte).  The lookup runs only for KEPT hashes:
// the window's position is parked beside the hash in the LDS list and resolved at the flush.  Then two radix sorts (by
// hash, then stably by segment), a flag / scan / write sequence, and the result is a CSR: mins[] strictly ascending inside
// each segment, abund[] their run lengths, off[n_seg + 1] -- mins and off are exactly what yh_db_create_device takes as
// d_values and d_offsets.
#include "yh_common.h"
#include "yh_sketch.h"

#include <algorithm>
#include <mutex>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

// (tests/test_gpu_sketch_edges.py restates SK_THREADS * SK_ITEMS, SK_LCAP, RL_RUN, RL_WIN and the 16-base unit: keep it in step)
constexpr int SK_THREADS = 256;
constexpr int SK_ITEMS = 8;      // windows per lane
constexpr int SK_LCAP = 2048;    // kept hashes parked in LDS per workgroup before the flush

__device__ __forceinline__ u64 rotl64(u64 x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ u64 fmix64(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// 0..3 for A,C,G,T (either case) in ALPHABETICAL order, 4 otherwise
__device__ __forceinline__ u32 base_code(u8 c) {
    const u32 u = c & 0xDFu;
    const bool ok = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T');
    const u32 x = (u >> 1) & 3u;  // A 0, C 1, T 2, G 3
    return ok ? (x ^ (x >> 1)) : 4u;  // -> A 0, C 1, G 2, T 3
}
__device__ __forceinline__ u8 code_ascii(u32 code) { return (u8)((0x54474341u >> (8 * code)) & 0xffu); }

// ---- segments (the SEG = true instantiations) ---------------------------------------------------------------------------------
// off[n_seg + 1] ascending byte offsets, n_seg >= 1; out_seg[] receives the segment of every hash stored in out[]
struct SegArgs {
    const u64* off;
    u32 n_seg;
    u32* out_seg;
};
constexpr u32 SEG_NONE = 0xffffffffu;

// the largest s in [lo, hi] with off[s] <= pos (lo when there is none): every read is inside off[lo .. hi], whatever the table holds
__device__ __forceinline__ u32 seg_find(const u64* __restrict__ off, u64 pos, u32 lo, u32 hi) {
    while (lo < hi) {
        const u32 m = lo + (hi - lo + 1u) / 2u;
        if (off[m] <= pos) lo = m; else hi = m - 1u;
    }
    return lo;
}
// the segment of the window that starts at pos (looked for in [lo, hi] <= n_seg - 1), SEG_NONE when its k bytes leave the segment
__device__ __forceinline__ u32 seg_of_window(const SegArgs& sa, u64 pos, u32 k, u32 lo, u32 hi) {
    const u32 s = seg_find(sa.off, pos, lo, hi);
    return (sa.off[s] <= pos && pos + k <= sa.off[s + 1]) ? s : SEG_NONE;
}
// the segments a workgroup's windows [first, last] can start in -> lrange[0 .. 1] (two lanes of two waves; before a barrier)
__device__ __forceinline__ void seg_range(const SegArgs& sa, u64 first, u64 last, u32* lrange) {
    if (threadIdx.x == 0) lrange[0] = seg_find(sa.off, first, 0u, sa.n_seg - 1u);
    if (threadIdx.x == 64) lrange[1] = seg_find(sa.off, last, 0u, sa.n_seg - 1u);
}

// A kept hash: into the workgroup's LDS list (SEG: with the position of its window, resolved at the flush), or, when the
// list is full, straight out (SEG: resolved here -- only this path pays a search per hash, and only at scaled close to 1).
template <bool SEG>
__device__ __forceinline__ void sk_keep(u64 h1, u64 pos, u32 k, u64* lbuf, u32* lpos, u32* lfill, const u32* lrange, const SegArgs& sa,
                                        u64 cap, u64* __restrict__ out, u64* __restrict__ out_count) {
    const u32 slot = atomicAdd(lfill, 1u);
    if (slot < (u32)SK_LCAP) {
        lbuf[slot] = h1;
        if constexpr (SEG) lpos[slot] = (u32)pos;
    } else {  // scaled close to 1: more kept hashes than the LDS list holds
        u32 s = 0;
        if constexpr (SEG) {
            s = seg_of_window(sa, pos, k, lrange[0], lrange[1]);
            if (s == SEG_NONE) return;
        }
        const u64 g = atomicAdd((unsigned long long*)out_count, 1ull);
        if (g < cap) {
            out[g] = h1;
            if constexpr (SEG) sa.out_seg[g] = s;
        }
    }
}
// The LDS list out, behind a barrier that follows the last sk_keep.  SEG: every entry's segment first (lanes in parallel,
// a search over the few segments of this workgroup's span), windows that leave their segment dropped, the rest compacted.
template <bool SEG, int THREADS>
__device__ __forceinline__ void sk_flush(u32 k, u64* lbuf, u32* lpos, u32* lfill, u32* lkept, u64* gbase, const u32* lrange, const SegArgs& sa,
                                         u64 cap, u64* __restrict__ out, u64* __restrict__ out_count) {
    const u32 f = min(*lfill, (u32)SK_LCAP);
    if (!f) return;
    if constexpr (!SEG) {
        if (threadIdx.x == 0) *gbase = atomicAdd((unsigned long long*)out_count, (unsigned long long)f);
        __syncthreads();
        for (u32 e = threadIdx.x; e < f; e += THREADS)
            if (*gbase + e < cap) out[*gbase + e] = lbuf[e];
    } else {
        u32 mine = 0;
        for (u32 e = threadIdx.x; e < f; e += THREADS) {
            const u32 s = seg_of_window(sa, (u64)lpos[e], k, lrange[0], lrange[1]);
            lpos[e] = s;
            mine += (s != SEG_NONE) ? 1u : 0u;
        }
        const u32 base = mine ? atomicAdd(lkept, mine) : 0u;
        __syncthreads();
        if (threadIdx.x == 0) *gbase = *lkept ? atomicAdd((unsigned long long*)out_count, (unsigned long long)*lkept) : 0ull;
        __syncthreads();
        u64 g = *gbase + base;
        for (u32 e = threadIdx.x; e < f; e += THREADS) {
            const u32 s = lpos[e];
            if (s == SEG_NONE) continue;
            if (g < cap) { out[g] = lbuf[e]; sa.out_seg[g] = s; }
            ++g;
        }
    }
}

// (win0: the first window of this launch -- a sequence that is still arriving is hashed piece by piece; n: bytes present)
template <bool SEG>
__global__ void __launch_bounds__(SK_THREADS) k_sketch_dna(const u8* __restrict__ seq, u64 n, u32 k, u64 seed,
                                                           u64 max_hash, u64 cap, u64* __restrict__ out,
                                                           u64* __restrict__ out_count, u64 win0, const SegArgs sa) {
    __shared__ u64 lbuf[SK_LCAP];
    __shared__ u32 lpos[SEG ? SK_LCAP : 1];
    __shared__ u32 lrange[2];
    __shared__ u32 lfill, lkept;
    __shared__ u64 gbase;
    if (threadIdx.x == 0) { lfill = 0; lkept = 0; }
    const u64 n_win = n - k + 1;
    const u64 block_first = win0 + (u64)blockIdx.x * SK_THREADS * SK_ITEMS;
    if constexpr (SEG) seg_range(sa, block_first, min(block_first + SK_THREADS * SK_ITEMS - 1, n - 1), lrange);
    __syncthreads();
    for (int it = 0; it < SK_ITEMS; ++it) {
        const u64 i = block_first + (u64)it * SK_THREADS + threadIdx.x;
        if (i >= n_win) continue;
        const u8* s = seq + i;
        // validity + orientation: the first position where the k-mer and its reverse complement
        // differ decides which one is canonical
        bool valid = true;
        int use_rc = -1;  // -1 undecided (so far equal)
        for (u32 j = 0; j < k; ++j) {
            const u32 a = base_code(s[j]);
            if (a > 3u) { valid = false; break; }
            if (use_rc < 0) {
                const u32 b = base_code(s[k - 1 - j]);
                if (b <= 3u && (3u - b) != a) use_rc = ((3u - b) < a) ? 1 : 0;
            }
        }
        if (!valid) continue;
        const bool rc = use_rc == 1;
        auto byte_at = [&](u32 j) -> u64 {
            const u32 c = rc ? 3u - base_code(s[k - 1 - j]) : base_code(s[j]);
            return (u64)code_ascii(c);
        };
        // MurmurHash3_x64_128, first word
        u64 h1 = seed, h2 = seed;
        const u64 c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
        const u32 nblocks = k / 16;
        for (u32 blk = 0; blk < nblocks; ++blk) {
            u64 k1 = 0, k2 = 0;
            for (u32 t = 0; t < 8; ++t) {
                k1 |= byte_at(16 * blk + t) << (8 * t);
                k2 |= byte_at(16 * blk + 8 + t) << (8 * t);
            }
            k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
            h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729ull;
            k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
            h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5ull;
        }
        const u32 tail = 16 * nblocks, rem = k - tail;
        if (rem > 8) {
            u64 k2 = 0;
            for (u32 t = 8; t < rem; ++t) k2 |= byte_at(tail + t) << (8 * (t - 8));
            k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
        }
        if (rem > 0) {
            u64 k1 = 0;
            for (u32 t = 0; t < (rem < 8 ? rem : 8u); ++t) k1 |= byte_at(tail + t) << (8 * t);
            k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
        }
        h1 ^= (u64)k; h2 ^= (u64)k;
        h1 += h2; h2 += h1;
        h1 = fmix64(h1); h2 = fmix64(h2);
        h1 += h2;
        if (h1 <= max_hash) sk_keep<SEG>(h1, i, k, lbuf, lpos, &lfill, lrange, sa, cap, out, out_count);
    }
    __syncthreads();
    sk_flush<SEG, SK_THREADS>(k, lbuf, lpos, &lfill, &lkept, &gbase, lrange, sa, cap, out, out_count);
}

// ---- k <= 64: the k-mer as a 2-bit string in one 64- or 128-bit word ---------------------------------------------------------
// The first kernel above reads every window's k bytes three times through L1 (23 G bases/s at k = 31: below what PCIe
// delivers).  Here a workgroup stages its 8 192 + k - 1 bases ONCE, coalesced, as 2-bit codes (16 bases per word, A C G T
// = 0 1 2 3) with one "not a base" bit each; a lane owns RL_RUN = 32 consecutive windows = 64 staged bases in four
// registers.  With the string packed little-endian (base j at bits 2j), window t is bits [2t, 2t + 2k) of it, its
// big-endian packing (the one whose numeric order is the lexicographic order) is kept by shifting one base in per window,
// and the reverse complement costs nothing:  BE(rc) = ~LE(fwd),  LE(rc) = ~BE(fwd)  (complement = 3 - code = ~code).
// The canonical k-mer's ASCII bytes, which MurmurHash3 wants, are spread out of the codes arithmetically, 8 bytes a time.
constexpr int RL_THREADS = 256;
constexpr int RL_RUN = 32;                         // windows per lane
constexpr int RL_WIN = RL_THREADS * RL_RUN;        // windows per workgroup
constexpr int RL_UNITS = RL_WIN / 16 + 4;          // staged 16-base units (the last lane reads six from its first)

// four bytes -> their 2-bit codes in the low bits of each byte, and bit 7 of a byte set when it is not A/C/G/T (either case)
__device__ __forceinline__ void codes_of4(u32 w, u32& codes, u32& bad) {
    const u32 x = w & 0xDFDFDFDFu;
    const u32 t = (x >> 1) & 0x03030303u;               // A 0, C 1, T 2, G 3
    const u32 c = t ^ ((t >> 1) & 0x01010101u);         // A 0, C 1, G 2, T 3
    const u32 lo = c & 0x01010101u, hi = (c >> 1) & 0x01010101u;
    const u32 expect = 0x41414141u + (lo & ~hi) * 2u + (hi & ~lo) * 6u + (lo & hi) * 0x13u;  // 'A' 'C' 'G' 'T'
    const u32 diff = x ^ expect;
    bad = (((diff & 0x7f7f7f7fu) + 0x7f7f7f7fu) | diff) & 0x80808080u;
    codes = c;
}
// 8 codes (16 bits, base j at bits 2j) -> 8 ASCII bytes (base j in byte j)
__device__ __forceinline__ u64 ascii_of8(u32 v16) {
    u64 x = v16;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    const u64 lo = x & 0x0101010101010101ull, hi = (x >> 1) & 0x0101010101010101ull;
    return 0x4141414141414141ull + (lo & ~hi) * 2ull + (hi & ~lo) * 6ull + (lo & hi) * 0x13ull;
}

typedef unsigned __int128 u128;
template <int KW> struct RollWord;
template <> struct RollWord<1> { typedef u64 type; };
template <> struct RollWord<2> { typedef u128 type; };
__device__ __forceinline__ u32 top_bit_plus1(u64 x) { return x ? 64u - (u32)__clzll((long long)x) : 0u; }
__device__ __forceinline__ u32 top_bit_plus1(u128 x) {
    const u64 h = (u64)(x >> 64);
    return h ? 64u + top_bit_plus1(h) : top_bit_plus1((u64)x);
}

// KW = 1: k <= 32, the k-mer in one 64-bit word; KW = 2: k <= 64, in a 128-bit one (the same code on a wider word)
// (SEG: the segmented form -- kept hashes leave with their segment, see sk_keep / sk_flush; the per-window loop is the same)
template <int KW, bool SEG>
__global__ void __launch_bounds__(RL_THREADS) k_sketch_dna_roll(const u8* __restrict__ seq, u64 n, u32 k, u64 seed,
                                                                u64 max_hash, u64 cap, u64* __restrict__ out,
                                                                u64* __restrict__ out_count, u64 win0, const SegArgs sa) {
    typedef typename RollWord<KW>::type word;
    constexpr u32 BITS = 64u * KW;      // of a word = 32 KW bases
    constexpr int NW = 4 * KW;          // 8-byte ASCII words of a k-mer
    __shared__ u32 lcode[RL_UNITS];
    __shared__ u32 lbad[RL_UNITS];
    __shared__ u64 lbuf[SK_LCAP];
    __shared__ u32 lpos[SEG ? SK_LCAP : 1];
    __shared__ u32 lrange[2];
    __shared__ u32 lfill, lkept;
    __shared__ u64 gbase;
    if (threadIdx.x == 0) { lfill = 0; lkept = 0; }
    const u64 n_win = n - k + 1;
    const u64 B0 = win0 + (u64)blockIdx.x * RL_WIN;  // first base (= first window) of the workgroup
    for (u32 u = threadIdx.x; u < (u32)RL_UNITS; u += RL_THREADS) {
        const u64 p = B0 + 16ull * u;
        u32 w[4] = {0u, 0u, 0u, 0u};  // (a zero byte is not a base)
        if (p + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(seq + p);  // (B0 and 16 u are multiples of 16)
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if (p < n) {
            for (u32 j = 0; j < 16 && p + j < n; ++j) w[j >> 2] |= (u32)seq[p + j] << (8 * (j & 3));
        }
        u32 codes = 0, bad = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u32 c, b;
            codes_of4(w[q], c, b);
            codes |= (((c * 0x41041u) >> 18) & 0xffu) << (8 * q);           // 4 codes -> 8 bits
            bad |= ((((b >> 7) * 0x00204081u) >> 21) & 0xfu) << (4 * q);    // 4 flags -> 4 bits
        }
        lcode[u] = codes;
        lbad[u] = bad;
    }
    if constexpr (SEG) seg_range(sa, B0, min(B0 + (u64)RL_WIN - 1, n - 1), lrange);
    __syncthreads();
    // the lane's 32 windows reach 32 + k - 1 <= 95 bases: units 2 l .. 2 l + 5 (six of sixteen bases; four when k <= 32)
    const u32 l2 = 2u * threadIdx.x;
    word P0 = 0, P1 = 0, bad = 0;
#pragma unroll
    for (int q = 0; q < 2 * KW; ++q) {
        P0 |= (word)lcode[l2 + q] << (32 * q);
        bad |= (word)lbad[l2 + q] << (16 * q);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        P1 |= (word)lcode[l2 + 2 * KW + q] << (32 * q);
        bad |= (word)lbad[l2 + 2 * KW + q] << (16 * (2 * KW + q));
    }
    const word one = 1;
    const word mask = (2 * k == BITS) ? ~(word)0 : ((one << (2 * k)) - one);
    const u64 w0 = B0 + (u64)threadIdx.x * RL_RUN;  // the lane's first window
    // big-endian packing of the first k - 1 bases (all in P0); the first window that no bad base among them reaches
    word fbe = 0;
    for (u32 j = 0; j + 1 < k; ++j) fbe = (fbe << 2) | ((P0 >> (2 * j)) & (word)3);
    const word head_bad = (k > 1) ? (bad & ((one << (k - 1)) - one)) : (word)0;
    u32 first_ok = top_bit_plus1(head_bad);
    const u64 c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
    const u32 nblocks = k / 16, rem = k & 15u;
    for (u32 t = 0; t < (u32)RL_RUN; ++t) {
        const u32 p = t + k - 1;                       // the base this window adds
        if ((u32)(bad >> p) & 1u) first_ok = p + 1;
        const word fle = (t ? ((P0 >> (2 * t)) | (P1 << (BITS - 2 * t))) : P0) & mask;
        fbe = ((fbe << 2) | ((fle >> (2 * (k - 1))) & (word)3)) & mask;
        if (t < first_ok || w0 + t >= n_win) continue;
        const word rbe = ~fle & mask;                  // BE(reverse complement)
        const word canon = (rbe < fbe) ? (~fbe & mask) : fle;   // LE packing of the canonical k-mer
        // its ASCII bytes, 8 per word, bytes from k on zero
        u64 W[NW];
#pragma unroll
        for (int m = 0; m < NW; ++m) {
            const int cnt = (int)k - 8 * m;            // bytes of this word
            u64 a = ascii_of8((u32)(canon >> (16 * m)) & 0xffffu);
            if (cnt <= 0) a = 0;
            else if (cnt < 8) a &= (1ull << (8 * cnt)) - 1ull;
            W[m] = a;
        }
        u64 h1 = seed, h2 = seed;
#pragma unroll
        for (int blk = 0; blk < NW / 2; ++blk) {
            if ((u32)blk < nblocks) {
                u64 k1 = W[2 * blk], k2 = W[2 * blk + 1];
                k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
                h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729ull;
                k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
                h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5ull;
            }
        }
        // the tail: the words behind the last whole block (zero when k is a multiple of 16)
        u64 t1 = 0, t2 = 0;
#pragma unroll
        for (int blk = 0; blk < NW / 2; ++blk)
            if ((u32)blk == nblocks) { t1 = W[2 * blk]; t2 = W[2 * blk + 1]; }
        if (rem > 8) { t2 *= c2; t2 = rotl64(t2, 33); t2 *= c1; h2 ^= t2; }
        if (rem > 0) { t1 *= c1; t1 = rotl64(t1, 31); t1 *= c2; h1 ^= t1; }
        h1 ^= (u64)k; h2 ^= (u64)k;
        h1 += h2; h2 += h1;
        h1 = fmix64(h1); h2 = fmix64(h2);
        h1 += h2;
        if (h1 <= max_hash) sk_keep<SEG>(h1, w0 + t, k, lbuf, lpos, &lfill, lrange, sa, cap, out, out_count);
    }
    __syncthreads();
    sk_flush<SEG, RL_THREADS>(k, lbuf, lpos, &lfill, &lkept, &gbase, lrange, sa, cap, out, out_count);
}

// The launch both entry points share: the windows [win0, win_end) of a sequence of which n_bytes are present (win0 a
// multiple of SK_WIN_ALIGN); k <= 64 through the 2-bit kernel (YH_SKETCH_BYTES=1 behind the tuning gate: the first one).
constexpr u64 SK_WIN_ALIGN = RL_WIN;  // (a multiple of both kernels' windows per workgroup)
static_assert(RL_WIN % (SK_THREADS * SK_ITEMS) == 0, "one alignment for both kernels");
// (sa: null = the plain form; else the segmented one, n_seg >= 1)
static int launch_sketch(const u8* d_seq, u64 n_bytes, u32 k, u64 seed, u64 max_hash, u64 cap, u64* d_out, u64* d_cnt, hipStream_t st,
                         u64 win0, u64 win_end, const SegArgs* sa = nullptr) {
    if (win_end <= win0) return YH_OK;
    static const bool bytes_only = yh_tune_flag("YH_SKETCH_BYTES");
    const bool roll = k <= 64 && !bytes_only && (reinterpret_cast<uintptr_t>(d_seq) & 15u) == 0;
    const u64 per_block = roll ? (u64)RL_WIN : (u64)SK_THREADS * SK_ITEMS;
    const u64 blocks = (win_end - win0 + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) { yh_set_error("sequence too long for one call"); return YH_ERR_INVALID_ARG; }
    const SegArgs none{nullptr, 0u, nullptr};
    if (sa) {
        if (roll && k <= 32) k_sketch_dna_roll<1, true><<<(u32)blocks, RL_THREADS, 0, st>>>(d_seq, n_bytes, k, seed, max_hash, cap, d_out, d_cnt, win0, *sa);
        else if (roll) k_sketch_dna_roll<2, true><<<(u32)blocks, RL_THREADS, 0, st>>>(d_seq, n_bytes, k, seed, max_hash, cap, d_out, d_cnt, win0, *sa);
        else k_sketch_dna<true><<<(u32)blocks, SK_THREADS, 0, st>>>(d_seq, n_bytes, k, seed, max_hash, cap, d_out, d_cnt, win0, *sa);
    } else if (roll && k <= 32) k_sketch_dna_roll<1, false><<<(u32)blocks, RL_THREADS, 0, st>>>(d_seq, n_bytes, k, seed, max_hash, cap, d_out, d_cnt, win0, none);
    else if (roll) k_sketch_dna_roll<2, false><<<(u32)blocks, RL_THREADS, 0, st>>>(d_seq, n_bytes, k, seed, max_hash, cap, d_out, d_cnt, win0, none);
    else k_sketch_dna<false><<<(u32)blocks, SK_THREADS, 0, st>>>(d_seq, n_bytes, k, seed, max_hash, cap, d_out, d_cnt, win0, none);
    YH_HIP(hipGetLastError());
    return YH_OK;
}

// ---- (segment, hash) pairs -> the sketches as a CSR --------------------------------------------------------------------------
// The pairs sit in cap slots; the first min(*n_kept, cap) are in (segment, hash) order after the two sorts, the slots nobody
// wrote hold the segment n_seg and sort behind them.  k_seg_heads flags the first pair of every run of equal pairs (one word
// per slot, and a zero behind the last); rocPRIM's exclusive scan of the flags is every slot's rank among the runs; k_seg_emit
// writes a run's hash and length at its rank; k_seg_off finds every segment's first pair by binary search and stores that
// pair's rank.  No atomic decides a position: the same input gives the same bytes.
constexpr u32 SG_THREADS = 256;

__global__ void __launch_bounds__(SG_THREADS) k_seg_heads(const u64* __restrict__ hash, const u32* __restrict__ seg, u64 cap,
                                                          const u64* __restrict__ n_kept, u32* __restrict__ flag) {
    const u64 i = (u64)blockIdx.x * SG_THREADS + threadIdx.x;
    if (i > cap) return;
    const u64 n = min(*n_kept, cap);
    flag[i] = (i < n && (i == 0 || seg[i] != seg[i - 1] || hash[i] != hash[i - 1])) ? 1u : 0u;
}

__global__ void __launch_bounds__(SG_THREADS) k_seg_emit(const u64* __restrict__ hash, const u32* __restrict__ seg, u64 cap,
                                                         const u64* __restrict__ n_kept, const u32* __restrict__ flag,
                                                         const u32* __restrict__ rank, u64 cap_mins, u64* __restrict__ mins,
                                                         u32* __restrict__ abund) {
    const u64 i = (u64)blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= cap || !flag[i]) return;
    const u64 r = rank[i];
    if (r >= cap_mins) return;
    const u64 n = min(*n_kept, cap);
    const u64 h = hash[i];
    const u32 s = seg[i];
    // the end of the run: the first pair behind i that differs (gallop, then bisect; most runs have one pair)
    u64 lo = i, step = 1;     // (lo: known equal)
    u64 hi = n;               // (hi: known different, or n)
    while (lo + step < n) {
        if (seg[lo + step] != s || hash[lo + step] != h) { hi = lo + step; break; }
        lo += step;
        step <<= 1;
    }
    while (lo + 1 < hi) {
        const u64 m = lo + (hi - lo) / 2;
        if (seg[m] == s && hash[m] == h) lo = m; else hi = m;
    }
    mins[r] = h;
    abund[r] = (u32)(hi - i);
}

// one lane per s in [0, n_seg]: off[s] = rank of the first pair whose segment is >= s; the last one is the total, also -> *n_distinct
__global__ void __launch_bounds__(SG_THREADS) k_seg_off(const u32* __restrict__ seg, u64 cap, const u64* __restrict__ n_kept,
                                                        const u32* __restrict__ rank, u32 n_seg, u64* __restrict__ off,
                                                        u64* __restrict__ n_distinct) {
    const u64 s = (u64)blockIdx.x * SG_THREADS + threadIdx.x;
    if (s > n_seg) return;
    const u64 n = min(*n_kept, cap);
    u64 lo = 0, hi = n;  // first i in [0, n] with seg[i] >= s
    while (lo < hi) {
        const u64 m = lo + (hi - lo) / 2;
        if ((u64)seg[m] < s) lo = m + 1; else hi = m;
    }
    const u64 r = rank[lo];  // (rank has cap + 1 entries: rank[n] = all the runs)
    off[s] = r;
    if (s == n_seg) *n_distinct = r;
}

// the layout of the work buffer of yh_sketch_segments_device for cap pairs (offsets in bytes, every part 256-byte aligned)
struct SegWork {
    u64 hash_a, hash_b, seg_a, seg_b, flag, rank, tmp, tmp_bytes, total;
};
static int seg_work_layout(u64 cap, SegWork& w) {
    size_t t1 = 0, t2 = 0, t3 = 0;
    if (cap) {
        YH_HIP(rocprim::radix_sort_pairs(nullptr, t1, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)cap, 0u, 64u, (hipStream_t) nullptr));
        YH_HIP(rocprim::radix_sort_pairs(nullptr, t2, (const u32*)nullptr, (u32*)nullptr, (const u64*)nullptr, (u64*)nullptr, (size_t)cap, 0u, 32u, (hipStream_t) nullptr));
    }
    YH_HIP(rocprim::exclusive_scan(nullptr, t3, (const u32*)nullptr, (u32*)nullptr, 0u, (size_t)cap + 1, rocprim::plus<u32>(), (hipStream_t) nullptr));
    auto up = [](u64 x) { return (x + 255ull) & ~255ull; };
    u64 at = 0;
    w.hash_a = at; at += up(cap * sizeof(u64));
    w.hash_b = at; at += up(cap * sizeof(u64));
    w.seg_a = at; at += up(cap * sizeof(u32));
    w.seg_b = at; at += up(cap * sizeof(u32));
    w.flag = at; at += up((cap + 1) * sizeof(u32));
    w.rank = at; at += up((cap + 1) * sizeof(u32));
    w.tmp = at;
    w.tmp_bytes = up(std::max<u64>(std::max<u64>(t1, t2), t3));
    w.total = at + w.tmp_bytes + 256;  // (+ 256: the caller's buffer need not be aligned)
    return YH_OK;
}
static u32 bits_of(u64 x) { u32 b = 1; while (b < 64 && (x >> b)) ++b; return b; }  // bits that hold x (at least one)

static int seg_args_ok(u64 n_bytes, u64 n_seg, int ksize) {
    if (ksize < 1 || ksize > 255) { yh_set_error("ksize must be in [1, 255]"); return YH_ERR_INVALID_ARG; }
    if (n_bytes >= (1ull << 32)) { yh_set_error("a segmented call takes less than 2^32 bytes"); return YH_ERR_INVALID_ARG; }
    if (n_seg >= (1ull << 32)) { yh_set_error("a segmented call takes less than 2^32 segments"); return YH_ERR_INVALID_ARG; }
    return YH_OK;
}

// Everything behind the upload, on st: d_totals zeroed, the windows [win0, win_end) hashed into the pairs (win0 = 0 for a
// resident sequence; the host form hashes the earlier windows itself, piece by piece, and passes hashed = true), sorted, cut.
static int seg_finish(const u8* d_seq, u64 n_bytes, const u64* d_seg_off, u32 n_seg, u32 k, u64 seed, u64 max_hash, u64 cap_kept,
                      u8* work, const SegWork& w, u64 cap_mins, u64* d_mins, u32* d_abund, u64* d_off, u64* d_totals, hipStream_t st,
                      bool hashed) {
    u64* hash_a = (u64*)(work + w.hash_a); u64* hash_b = (u64*)(work + w.hash_b);
    u32* seg_a = (u32*)(work + w.seg_a); u32* seg_b = (u32*)(work + w.seg_b);
    u32* flag = (u32*)(work + w.flag); u32* rank = (u32*)(work + w.rank);
    if (!hashed) {
        YH_HIP(hipMemsetAsync(d_totals, 0, 2 * sizeof(u64), st));
        if (cap_kept) YH_HIP(hipMemsetD32Async((hipDeviceptr_t)seg_a, (int)n_seg, cap_kept, st));
        if (n_bytes >= k) {
            const SegArgs sa{d_seg_off, n_seg, seg_a};
            YH_TRY(launch_sketch(d_seq, n_bytes, k, seed, max_hash, cap_kept, hash_a, d_totals, st, 0, n_bytes - k + 1, &sa));
        }
    }
    if (cap_kept) {
        size_t tb = w.tmp_bytes;
        YH_HIP(rocprim::radix_sort_pairs(work + w.tmp, tb, (const u64*)hash_a, hash_b, (const u32*)seg_a, seg_b, (size_t)cap_kept, 0u, bits_of(max_hash), st));
        tb = w.tmp_bytes;
        YH_HIP(rocprim::radix_sort_pairs(work + w.tmp, tb, (const u32*)seg_b, seg_a, (const u64*)hash_b, hash_a, (size_t)cap_kept, 0u, bits_of(n_seg), st));  // stable: hashes stay ascending inside a segment
    }
    k_seg_heads<<<(u32)((cap_kept + 1 + SG_THREADS - 1) / SG_THREADS), SG_THREADS, 0, st>>>(hash_a, seg_a, cap_kept, d_totals, flag);
    size_t tb = w.tmp_bytes;
    YH_HIP(rocprim::exclusive_scan(work + w.tmp, tb, (const u32*)flag, rank, 0u, (size_t)cap_kept + 1, rocprim::plus<u32>(), st));
    if (cap_kept && cap_mins) k_seg_emit<<<(u32)((cap_kept + SG_THREADS - 1) / SG_THREADS), SG_THREADS, 0, st>>>(hash_a, seg_a, cap_kept, d_totals, flag, rank, cap_mins, d_mins, d_abund);
    k_seg_off<<<(u32)(((u64)n_seg + 1 + SG_THREADS - 1) / SG_THREADS), SG_THREADS, 0, st>>>(seg_a, cap_kept, d_totals, rank, n_seg, d_off, d_totals + 1);
    YH_HIP(hipGetLastError());
    return YH_OK;
}

// ---- the accumulator's compaction (yh_sketch_acc*, at the end of the file) -----------------------------------------------------
// n (key, count) pairs sorted by key -> one pair per distinct key with the counts summed.  As above: k_acc_heads flags the
// first pair of every run of equal keys (and puts a zero behind the last flag and the last count), one exclusive scan of
// the flags is every run's rank, one exclusive u64 scan of the counts gives pre[0 .. n], k_acc_emit writes a run's key at its
// rank and pre[end] - pre[begin] as its count.  One lane per pair; no lane walks a run, no atomic decides a position.
__global__ void __launch_bounds__(SG_THREADS) k_acc_ones(u64* __restrict__ cnt, u64 n) {
    const u64 i = (u64)blockIdx.x * SG_THREADS + threadIdx.x;
    if (i < n) cnt[i] = 1ull;
}

// (flag and cnt have n + 1 entries)
__global__ void __launch_bounds__(SG_THREADS) k_acc_heads(const u64* __restrict__ key, u64 n, u32* __restrict__ flag, u64* __restrict__ cnt) {
    const u64 i = (u64)blockIdx.x * SG_THREADS + threadIdx.x;
    if (i > n) return;
    if (i == n) { flag[i] = 0u; cnt[i] = 0ull; return; }
    flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(SG_THREADS) k_acc_emit(const u64* __restrict__ key, u64 n, const u32* __restrict__ flag,
                                                         const u32* __restrict__ rank, const u64* __restrict__ pre,
                                                         u64* __restrict__ key_out, u64* __restrict__ cnt_out) {
    const u64 i = (u64)blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const u64 h = key[i];
    // the end of the run: the first pair behind i with another key (gallop, then bisect; most runs have one pair)
    u64 lo = i, step = 1;     // (lo: known equal)
    u64 hi = n;               // (hi: known different, or n)
    while (lo + step < n) {
        if (key[lo + step] != h) { hi = lo + step; break; }
        lo += step;
        step <<= 1;
    }
    while (lo + 1 < hi) {
        const u64 m = lo + (hi - lo) / 2;
        if (key[m] == h) lo = m; else hi = m;
    }
    const u64 r = rank[i];    // (r <= i)
    key_out[r] = h;
    cnt_out[r] = pre[hi] - pre[i];
}

}  // namespace

// device buffers, enqueued on `stream`: *d_count is zeroed first and receives the number of kept hashes (which may exceed
// cap: then only the first cap were stored)
extern "C" int yh_sketch_dna_device(const uint8_t* d_seq, uint64_t n_bytes, int ksize, uint64_t seed, uint64_t max_hash,
                                    uint64_t cap, uint64_t* d_hashes_out, uint64_t* d_count, void* stream) {
    if (!d_count || (cap && !d_hashes_out) || (n_bytes && !d_seq)) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    if (ksize < 1 || ksize > 255) { yh_set_error("ksize must be in [1, 255]"); return YH_ERR_INVALID_ARG; }
    hipStream_t st = (hipStream_t)stream;
    YH_HIP(hipMemsetAsync(d_count, 0, sizeof(u64), st));
    if (n_bytes < (uint64_t)ksize) return YH_OK;
    YH_TRY(launch_sketch(d_seq, n_bytes, (u32)ksize, seed, max_hash, cap, (u64*)d_hashes_out, (u64*)d_count, st, 0, n_bytes - (u64)ksize + 1));
    return YH_OK;
}

extern "C" int yh_sketch_dna(const uint8_t* seq, uint64_t n_bytes, int ksize, uint64_t seed, uint64_t max_hash,
                             int device_id, uint64_t cap, uint64_t* hashes_out, uint64_t* n_out) {
    if (!n_out || (cap && !hashes_out) || (n_bytes && !seq)) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    if (ksize < 1 || ksize > 255) { yh_set_error("ksize must be in [1, 255]"); return YH_ERR_INVALID_ARG; }
    *n_out = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        yh_set_error("no HIP device available (libyacht_hip has no CPU fallback)");
        return YH_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { yh_set_error("device_id %d out of range", device_id); return YH_ERR_NO_DEVICE; }
    YH_HIP(hipSetDevice(device_id));
    if (n_bytes < (uint64_t)ksize) return YH_OK;
    // The sequence goes up in pieces of 32 MiB on one stream while the windows that are complete are hashed on another
    // (the kernel runs at ~2.5 x the bus: the call costs the upload plus the last piece); buffers, streams and events are
    // kept per device between calls (up to 1 GiB of sequence), one call per process at a time.
    struct SkCtx { u8* d_seq = nullptr; u64 seq_cap = 0; u64* d_out = nullptr; u64 out_cap = 0; u64* d_cnt = nullptr;
                   hipStream_t s_copy = nullptr, s_comp = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; };
    static std::mutex mu;
    static SkCtx ctxs[64];
    std::lock_guard<std::mutex> lock(mu);
    SkCtx& c = ctxs[device_id & 63];
    int rc = YH_OK;
#define SK_HIP(call)                                                              \
    if (rc == YH_OK) {                                                            \
        hipError_t e__ = (call);                                                  \
        if (e__ != hipSuccess) {                                                  \
            yh_set_error("%s failed: %s", #call, hipGetErrorString(e__));         \
            rc = (e__ == hipErrorOutOfMemory) ? YH_ERR_OOM : YH_ERR_HIP;          \
        }                                                                         \
    }
    if (!c.s_copy) {
        SK_HIP(hipStreamCreateWithFlags(&c.s_copy, hipStreamNonBlocking));
        SK_HIP(hipStreamCreateWithFlags(&c.s_comp, hipStreamNonBlocking));
        SK_HIP(hipEventCreateWithFlags(&c.ev[0], hipEventDisableTiming));
        SK_HIP(hipEventCreateWithFlags(&c.ev[1], hipEventDisableTiming));
        SK_HIP(hipMalloc((void**)&c.d_cnt, sizeof(u64)));
    }
    if (rc == YH_OK && c.seq_cap < n_bytes) {
        if (c.d_seq) (void)hipFree(c.d_seq);
        c.d_seq = nullptr; c.seq_cap = 0;
        SK_HIP(hipMalloc((void**)&c.d_seq, n_bytes + 64));
        if (rc == YH_OK) c.seq_cap = n_bytes;
    }
    if (rc == YH_OK && c.out_cap < std::max<u64>(cap, 1)) {
        if (c.d_out) (void)hipFree(c.d_out);
        c.d_out = nullptr; c.out_cap = 0;
        SK_HIP(hipMalloc((void**)&c.d_out, std::max<u64>(cap, 1) * sizeof(u64)));
        if (rc == YH_OK) c.out_cap = std::max<u64>(cap, 1);
    }
    SK_HIP(hipMemsetAsync(c.d_cnt, 0, sizeof(u64), c.s_comp));
    const u64 n_win = n_bytes - (u64)ksize + 1;
    const u64 piece = 32ull << 20;
    u64 done_win = 0;
    int flip = 0;
    for (u64 p0 = 0; p0 < n_bytes && rc == YH_OK; p0 += piece, flip ^= 1) {
        const u64 p1 = std::min<u64>(n_bytes, p0 + piece);
        SK_HIP(hipMemcpyAsync(c.d_seq + p0, seq + p0, p1 - p0, hipMemcpyHostToDevice, c.s_copy));  // (pageable: returns when the piece has left the host)
        SK_HIP(hipEventRecord(c.ev[flip], c.s_copy));
        SK_HIP(hipStreamWaitEvent(c.s_comp, c.ev[flip], 0));
        // windows whose bytes are all there, in whole workgroups (the last piece: all that is left)
        u64 avail = p1 >= (u64)ksize ? p1 - (u64)ksize + 1 : 0;
        u64 upto = (p1 == n_bytes) ? n_win : (avail / SK_WIN_ALIGN) * SK_WIN_ALIGN;
        if (rc == YH_OK && upto > done_win) {
            rc = launch_sketch(c.d_seq, p1, (u32)ksize, seed, max_hash, cap, c.d_out, c.d_cnt, c.s_comp, done_win, upto);
            done_win = upto;
        }
    }
    u64 total = 0;
    SK_HIP(hipMemcpyAsync(&total, c.d_cnt, sizeof(u64), hipMemcpyDeviceToHost, c.s_comp));
    SK_HIP(hipStreamSynchronize(c.s_comp));
    if (rc == YH_OK) {
        *n_out = total;
        if (total > cap) {
            if (cap) { yh_set_error("hash buffer holds %llu entries, %llu needed", (u64)cap, total); rc = YH_ERR_CAPACITY; }
        } else if (total) {
            SK_HIP(hipMemcpyAsync(hashes_out, c.d_out, total * sizeof(u64), hipMemcpyDeviceToHost, c.s_comp));
            SK_HIP(hipStreamSynchronize(c.s_comp));
        }
    }
    if (rc != YH_OK) { (void)hipStreamSynchronize(c.s_copy); (void)hipStreamSynchronize(c.s_comp); }
#undef SK_HIP
    if (c.seq_cap > (1ull << 30)) { (void)hipFree(c.d_seq); c.d_seq = nullptr; c.seq_cap = 0; }
    return rc;
}

// ---- the segmented form -------------------------------------------------------------------------------------------------------
extern "C" uint64_t yh_sketch_segments_work_bytes(uint64_t cap_kept, uint64_t n_seg) {
    (void)n_seg;  // (the layout depends on the pairs alone; the argument is there so that it may)
    SegWork w;
    if (seg_work_layout(std::min<u64>(cap_kept, 0xffffffffull), w) != YH_OK) return 0;
    return w.total;
}

extern "C" int yh_sketch_segments_device(const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* d_seg_off, uint64_t n_seg, int ksize,
                                         uint64_t seed, uint64_t max_hash, uint64_t cap_kept, void* d_work, uint64_t work_bytes,
                                         uint64_t cap_mins, uint64_t* d_mins, uint32_t* d_abund, uint64_t* d_off, uint64_t* d_totals,
                                         void* stream) {
    if (!d_seg_off || !d_off || !d_totals || !d_work || (n_bytes && !d_seq) || (cap_mins && (!d_mins || !d_abund))) {
        yh_set_error("null argument");
        return YH_ERR_INVALID_ARG;
    }
    YH_TRY(seg_args_ok(n_bytes, n_seg, ksize));
    hipStream_t st = (hipStream_t)stream;
    if (n_seg == 0) {
        YH_HIP(hipMemsetAsync(d_totals, 0, 2 * sizeof(u64), st));
        YH_HIP(hipMemsetAsync(d_off, 0, sizeof(u64), st));
        return YH_OK;
    }
    cap_kept = std::min<u64>(cap_kept, n_bytes);  // (never more pairs than windows)
    SegWork w;
    YH_TRY(seg_work_layout(cap_kept, w));
    if (work_bytes < w.total) { yh_set_error("work buffer holds %llu bytes, %llu needed", (u64)work_bytes, w.total); return YH_ERR_INVALID_ARG; }
    u8* work = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(d_work) + 255u) & ~(uintptr_t)255u);
    return seg_finish(d_seq, n_bytes, (const u64*)d_seg_off, (u32)n_seg, (u32)ksize, seed, max_hash, cap_kept, work, w, cap_mins,
                      (u64*)d_mins, d_abund, (u64*)d_off, (u64*)d_totals, st, false);
}

extern "C" int yh_sketch_segments(const uint8_t* seq, uint64_t n_bytes, const uint64_t* seg_off, uint64_t n_seg, int ksize, uint64_t seed,
                                  uint64_t max_hash, int device_id, uint64_t cap_mins, uint64_t* mins_out, uint32_t* abund_out,
                                  uint64_t* off_out, uint64_t* n_out) {
    if (!n_out || !seg_off || !off_out || (n_bytes && !seq) || (cap_mins && (!mins_out || !abund_out))) {
        yh_set_error("null argument");
        return YH_ERR_INVALID_ARG;
    }
    *n_out = 0;
    YH_TRY(seg_args_ok(n_bytes, n_seg, ksize));
    if (seg_off[0] != 0 || seg_off[n_seg] != n_bytes) { yh_set_error("segment offsets must start at 0 and end at n_bytes"); return YH_ERR_INVALID_ARG; }
    for (u64 s = 0; s < n_seg; ++s)
        if (seg_off[s] > seg_off[s + 1]) { yh_set_error("segment offsets must not descend (segment %llu)", s); return YH_ERR_INVALID_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        yh_set_error("no HIP device available (libyacht_hip has no CPU fallback)");
        return YH_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { yh_set_error("device_id %d out of range", device_id); return YH_ERR_NO_DEVICE; }
    YH_HIP(hipSetDevice(device_id));
    for (u64 s = 0; s <= n_seg; ++s) off_out[s] = 0;
    if (n_seg == 0 || n_bytes < (uint64_t)ksize) return YH_OK;
    // As yh_sketch_dna: the sequence goes up in pieces of 32 MiB on one stream while the complete windows are hashed on
    // another; buffers, streams and events are kept per device between calls.  The pairs get room for 1.25 x the expected
    // number of kept hashes (+ 4 096); a sequence that keeps more (low complexity) is hashed once more, from HBM, with room
    // for the count the first pass reported.
    struct SgCtx { u8* d_seq = nullptr; u64 seq_cap = 0; u64* d_segoff = nullptr; u64 seg_cap = 0; u8* d_work = nullptr; u64 work_cap = 0;
                   u64* d_mins = nullptr; u32* d_abund = nullptr; u64 out_cap = 0; u64* d_off = nullptr; u64 off_cap = 0; u64* d_tot = nullptr;
                   hipStream_t s_copy = nullptr, s_comp = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; };
    static std::mutex mu;
    static SgCtx ctxs[64];
    std::lock_guard<std::mutex> lock(mu);
    SgCtx& c = ctxs[device_id & 63];
    int rc = YH_OK;
#define SK_HIP(call)                                                              \
    if (rc == YH_OK) {                                                            \
        hipError_t e__ = (call);                                                  \
        if (e__ != hipSuccess) {                                                  \
            yh_set_error("%s failed: %s", #call, hipGetErrorString(e__));         \
            rc = (e__ == hipErrorOutOfMemory) ? YH_ERR_OOM : YH_ERR_HIP;          \
        }                                                                         \
    }
#define SK_GROW(ptr, have, want, bytes)                                           \
    if (rc == YH_OK && (have) < (want)) {                                         \
        if (ptr) (void)hipFree(ptr);                                              \
        ptr = nullptr; have = 0;                                                  \
        SK_HIP(hipMalloc((void**)&ptr, (bytes)));                                 \
        if (rc == YH_OK) have = (want);                                           \
    }
    if (!c.s_copy) {
        SK_HIP(hipStreamCreateWithFlags(&c.s_copy, hipStreamNonBlocking));
        SK_HIP(hipStreamCreateWithFlags(&c.s_comp, hipStreamNonBlocking));
        SK_HIP(hipEventCreateWithFlags(&c.ev[0], hipEventDisableTiming));
        SK_HIP(hipEventCreateWithFlags(&c.ev[1], hipEventDisableTiming));
        SK_HIP(hipMalloc((void**)&c.d_tot, 2 * sizeof(u64)));
    }
    const u64 n_win = n_bytes - (u64)ksize + 1;
    const double keep = ((double)max_hash + 1.0) / 18446744073709551616.0;
    u64 cap_kept = std::min<u64>(n_win, (u64)((double)n_win * keep * 1.25) + 4096);
    SK_GROW(c.d_seq, c.seq_cap, n_bytes, n_bytes + 64);
    SK_GROW(c.d_segoff, c.seg_cap, n_seg + 1, (n_seg + 1) * sizeof(u64));
    SK_GROW(c.d_off, c.off_cap, n_seg + 1, (n_seg + 1) * sizeof(u64));
    u64 totals[2] = {0, 0};
    for (int pass = 0; pass < 2 && rc == YH_OK; ++pass) {
        SegWork w;
        if (rc == YH_OK) rc = seg_work_layout(cap_kept, w);
        SK_GROW(c.d_work, c.work_cap, w.total, w.total);
        if (rc == YH_OK && c.out_cap < cap_kept) {
            if (c.d_mins) (void)hipFree(c.d_mins);
            if (c.d_abund) (void)hipFree(c.d_abund);
            c.d_mins = nullptr; c.d_abund = nullptr; c.out_cap = 0;
            SK_HIP(hipMalloc((void**)&c.d_mins, cap_kept * sizeof(u64)));
            SK_HIP(hipMalloc((void**)&c.d_abund, cap_kept * sizeof(u32)));
            if (rc == YH_OK) c.out_cap = cap_kept;
        }
        if (rc != YH_OK) break;
        u8* work = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(c.d_work) + 255u) & ~(uintptr_t)255u);
        const SegArgs sa{c.d_segoff, (u32)n_seg, (u32*)(work + w.seg_a)};
        SK_HIP(hipMemsetAsync(c.d_tot, 0, 2 * sizeof(u64), c.s_comp));
        SK_HIP(hipMemsetD32Async((hipDeviceptr_t)sa.out_seg, (int)(u32)n_seg, cap_kept, c.s_comp));
        if (pass == 0) {
            SK_HIP(hipMemcpyAsync(c.d_segoff, seg_off, (n_seg + 1) * sizeof(u64), hipMemcpyHostToDevice, c.s_comp));
            const u64 piece = 32ull << 20;
            u64 done_win = 0;
            int flip = 0;
            for (u64 p0 = 0; p0 < n_bytes && rc == YH_OK; p0 += piece, flip ^= 1) {
                const u64 p1 = std::min<u64>(n_bytes, p0 + piece);
                SK_HIP(hipMemcpyAsync(c.d_seq + p0, seq + p0, p1 - p0, hipMemcpyHostToDevice, c.s_copy));
                SK_HIP(hipEventRecord(c.ev[flip], c.s_copy));
                SK_HIP(hipStreamWaitEvent(c.s_comp, c.ev[flip], 0));
                // windows whose bytes are all there, in whole workgroups (the last piece: all that is left)
                const u64 avail = p1 >= (u64)ksize ? p1 - (u64)ksize + 1 : 0;
                const u64 upto = (p1 == n_bytes) ? n_win : (avail / SK_WIN_ALIGN) * SK_WIN_ALIGN;
                if (rc == YH_OK && upto > done_win) {
                    rc = launch_sketch(c.d_seq, p1, (u32)ksize, seed, max_hash, cap_kept, (u64*)(work + w.hash_a), c.d_tot, c.s_comp, done_win, upto, &sa);
                    done_win = upto;
                }
            }
        } else if (rc == YH_OK) {
            rc = launch_sketch(c.d_seq, n_bytes, (u32)ksize, seed, max_hash, cap_kept, (u64*)(work + w.hash_a), c.d_tot, c.s_comp, 0, n_win, &sa);
        }
        if (rc == YH_OK)
            rc = seg_finish(c.d_seq, n_bytes, c.d_segoff, (u32)n_seg, (u32)ksize, seed, max_hash, cap_kept, work, w, cap_kept, c.d_mins, c.d_abund,
                            c.d_off, c.d_tot, c.s_comp, true);
        SK_HIP(hipMemcpyAsync(totals, c.d_tot, 2 * sizeof(u64), hipMemcpyDeviceToHost, c.s_comp));
        SK_HIP(hipStreamSynchronize(c.s_comp));
        if (rc != YH_OK || totals[0] <= cap_kept) break;
        if (pass == 1) { yh_set_error("kept hashes changed between two passes"); rc = YH_ERR_HIP; break; }
        cap_kept = totals[0];
    }
    if (rc == YH_OK) {
        *n_out = totals[1];
        SK_HIP(hipMemcpyAsync(off_out, c.d_off, (n_seg + 1) * sizeof(u64), hipMemcpyDeviceToHost, c.s_comp));
        if (cap_mins && totals[1] <= cap_mins && totals[1]) {
            SK_HIP(hipMemcpyAsync(mins_out, c.d_mins, totals[1] * sizeof(u64), hipMemcpyDeviceToHost, c.s_comp));
            SK_HIP(hipMemcpyAsync(abund_out, c.d_abund, totals[1] * sizeof(u32), hipMemcpyDeviceToHost, c.s_comp));
        }
        SK_HIP(hipStreamSynchronize(c.s_comp));
        if (rc == YH_OK && cap_mins && totals[1] > cap_mins) {
            yh_set_error("sketch buffers hold %llu entries, %llu needed", (u64)cap_mins, totals[1]);
            rc = YH_ERR_CAPACITY;
        }
    }
    if (rc != YH_OK && rc != YH_ERR_CAPACITY) { (void)hipStreamSynchronize(c.s_copy); (void)hipStreamSynchronize(c.s_comp); }
#undef SK_GROW
#undef SK_HIP
    if (c.seq_cap > (1ull << 30)) { (void)hipFree(c.d_seq); c.d_seq = nullptr; c.seq_cap = 0; }
    return rc;
}

// The hashing and the finish of yh_sketch_segments on the caller's buffers and streams (yh_sketch.h): what yh_classify_segments
// runs in front of the lookup, so that the sketches stay in HBM.  (yh_sketch_segments keeps its own loop over its own per-device
// buffers: the two differ in who owns the buffers and the streams, not in the order of the steps.)
int yh_q_sketch_segments_hosted(const u8* seq, u64 n_bytes, u8* d_seq, const u64* d_seg_off, u32 n_seg, u32 ksize, u64 seed, u64 max_hash,
                                u64 cap_kept, void* d_work, u64* d_mins, u32* d_abund, u64* d_off, u64* d_totals, hipStream_t s_comp,
                                hipStream_t s_copy, hipEvent_t ev[2], bool upload) {
    SegWork w;
    YH_TRY(seg_work_layout(cap_kept, w));
    u8* work = reinterpret_cast<u8*>((reinterpret_cast<uintptr_t>(d_work) + 255u) & ~(uintptr_t)255u);
    const SegArgs sa{d_seg_off, n_seg, (u32*)(work + w.seg_a)};
    const u64 n_win = n_bytes - (u64)ksize + 1;
    YH_HIP(hipMemsetAsync(d_totals, 0, 2 * sizeof(u64), s_comp));
    if (cap_kept) YH_HIP(hipMemsetD32Async((hipDeviceptr_t)sa.out_seg, (int)n_seg, cap_kept, s_comp));
    if (upload) {
        const u64 piece = 32ull << 20;
        u64 done_win = 0;
        int flip = 0;
        for (u64 p0 = 0; p0 < n_bytes; p0 += piece, flip ^= 1) {
            const u64 p1 = std::min<u64>(n_bytes, p0 + piece);
            YH_HIP(hipMemcpyAsync(d_seq + p0, seq + p0, p1 - p0, hipMemcpyHostToDevice, s_copy));
            YH_HIP(hipEventRecord(ev[flip], s_copy));
            YH_HIP(hipStreamWaitEvent(s_comp, ev[flip], 0));
            // windows whose bytes are all there, in whole workgroups (the last piece: all that is left)
            const u64 avail = p1 >= (u64)ksize ? p1 - (u64)ksize + 1 : 0;
            const u64 upto = (p1 == n_bytes) ? n_win : (avail / SK_WIN_ALIGN) * SK_WIN_ALIGN;
            if (upto > done_win) {
                YH_TRY(launch_sketch(d_seq, p1, ksize, seed, max_hash, cap_kept, (u64*)(work + w.hash_a), d_totals, s_comp, done_win, upto, &sa));
                done_win = upto;
            }
        }
    } else {
        YH_TRY(launch_sketch(d_seq, n_bytes, ksize, seed, max_hash, cap_kept, (u64*)(work + w.hash_a), d_totals, s_comp, 0, n_win, &sa));
    }
    return seg_finish(d_seq, n_bytes, d_seg_off, n_seg, ksize, seed, max_hash, cap_kept, work, w, cap_kept, d_mins, d_abund, d_off, d_totals,
                      s_comp, true);
}

// ---- the accumulator: one sketch with abundances out of many chunks -----------------------------------------------------------
// The state is a LOG: key[capacity] / cnt[capacity]; entries [0, n_compacted) are strictly ascending distinct hashes with their
// counts, entries [n_compacted, n_entries) raw kept hashes in arrival order.  A chunk is hashed by launch_sketch straight
// behind the tail; a full log is compacted (sort by key, flag / scan / emit: k_acc_* above) and, when fewer than D entries
// stay free behind the D distinct ones, doubled.  Counts of raw entries are implied (1) and written only when a compaction
// or yh_sketch_acc_add_hashes needs them: cnt is valid in [0, n_filled).  The result depends on the multiset of kept hashes
// alone -- not on the chunking, the capacity or the moments of compaction.  One call at a time per handle.
constexpr u64 ACC_DEFAULT_CAP = 1ull << 21;
constexpr u64 ACC_MAX_CAP = 0xfffffffeull;  // (flags and ranks are 32-bit words, one more than the entries)

struct yh_sketch_acc {
    int device = -1;
    u32 k = 0;
    u64 seed = 0, max_hash = 0;
    hipStream_t s_copy = nullptr, s_comp = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    u64* key = nullptr;
    u64* cnt = nullptr;
    u64 capacity = 0, n_entries = 0, n_compacted = 0, n_filled = 0;
    // scratch of a compaction, for work_cap pairs: the sorted pairs, flags, ranks, prefix sums (+ 1 each), rocPRIM's storage
    u8* work = nullptr;
    u64 work_cap = 0;
    u64 *key_b = nullptr, *cnt_b = nullptr, *pre = nullptr;
    u32 *flag = nullptr, *rank = nullptr;
    void* tmp = nullptr;
    u64 tmp_bytes = 0;
    u8* d_seq = nullptr;   // the chunk of a host-form add
    u64 seq_cap = 0;
    u64* d_cnt = nullptr;  // the hashing kernels' append counter
    u64 n_bytes = 0, n_kept = 0, n_compactions = 0, n_rehashed = 0;
};

static bool acc_ok(yh_sketch_acc* a) {
    if (!a) { yh_set_error("null yh_sketch_acc handle"); return false; }
    return true;
}

static u32 acc_blocks(u64 n) { return (u32)((n + SG_THREADS - 1) / SG_THREADS); }

// key / cnt for newcap entries, the first n_entries kept
static int acc_grow(yh_sketch_acc* a, u64 newcap) {
    if (newcap > ACC_MAX_CAP) { yh_set_error("the accumulator holds at most %llu entries", ACC_MAX_CAP); return YH_ERR_UNSUPPORTED; }
    newcap = std::max<u64>(newcap, 1);
    u64 *nk = nullptr, *nc = nullptr;
    YH_HIP(hipMalloc((void**)&nk, newcap * sizeof(u64)));
    hipError_t e = hipMalloc((void**)&nc, newcap * sizeof(u64));
    if (e == hipSuccess && a->n_entries) {
        e = hipMemcpyAsync(nk, a->key, a->n_entries * sizeof(u64), hipMemcpyDeviceToDevice, a->s_comp);
        if (e == hipSuccess && a->n_filled) e = hipMemcpyAsync(nc, a->cnt, a->n_filled * sizeof(u64), hipMemcpyDeviceToDevice, a->s_comp);
        if (e == hipSuccess) e = hipStreamSynchronize(a->s_comp);
    }
    if (e != hipSuccess) {
        (void)hipFree(nk);
        if (nc) (void)hipFree(nc);
        yh_set_error("growing the accumulator to %llu entries failed: %s", newcap, hipGetErrorString(e));
        return (e == hipErrorOutOfMemory) ? YH_ERR_OOM : YH_ERR_HIP;
    }
    if (a->key) (void)hipFree(a->key);
    if (a->cnt) (void)hipFree(a->cnt);
    a->key = nk; a->cnt = nc; a->capacity = newcap;
    return YH_OK;
}

// the scratch arrays for `pairs` pairs
static int acc_work(yh_sketch_acc* a, u64 pairs) {
    if (a->work_cap >= pairs) return YH_OK;
    if (a->work) (void)hipFree(a->work);
    a->work = nullptr; a->work_cap = 0;
    auto up = [](u64 x) { return (x + 255ull) & ~255ull; };
    const u64 b64 = up((pairs + 1) * sizeof(u64)), b32 = up((pairs + 1) * sizeof(u32));
    YH_HIP(hipMalloc((void**)&a->work, 3 * b64 + 2 * b32));
    a->key_b = (u64*)a->work;
    a->cnt_b = (u64*)(a->work + b64);
    a->pre = (u64*)(a->work + 2 * b64);
    a->flag = (u32*)(a->work + 3 * b64);
    a->rank = (u32*)(a->work + 3 * b64 + b32);
    a->work_cap = pairs;
    return YH_OK;
}

// The log -> distinct ascending hashes with summed counts (n_entries = n_compacted afterwards); then the growth rule: at
// least as many free entries as distinct ones.  One synchronize (the number of distinct hashes comes back).
static int acc_compact(yh_sketch_acc* a) {
    const u64 n = a->n_entries;
    if (n == a->n_compacted) return YH_OK;
    hipStream_t st = a->s_comp;
    YH_TRY(acc_work(a, a->capacity));
    size_t t1 = 0, t2 = 0, t3 = 0;
    const u32 bits = bits_of(a->max_hash);
    YH_HIP(rocprim::radix_sort_pairs(nullptr, t1, (const u64*)nullptr, (u64*)nullptr, (const u64*)nullptr, (u64*)nullptr, (size_t)n, 0u, bits, st));
    YH_HIP(rocprim::exclusive_scan(nullptr, t2, (const u32*)nullptr, (u32*)nullptr, 0u, (size_t)n + 1, rocprim::plus<u32>(), st));
    YH_HIP(rocprim::exclusive_scan(nullptr, t3, (const u64*)nullptr, (u64*)nullptr, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), st));
    const u64 need = std::max<u64>(std::max<u64>(t1, t2), std::max<u64>(t3, 256));
    if (a->tmp_bytes < need) {
        if (a->tmp) (void)hipFree(a->tmp);
        a->tmp = nullptr; a->tmp_bytes = 0;
        YH_HIP(hipMalloc(&a->tmp, need));
        a->tmp_bytes = need;
    }
    if (a->n_filled < n) k_acc_ones<<<acc_blocks(n - a->n_filled), SG_THREADS, 0, st>>>(a->cnt + a->n_filled, n - a->n_filled);
    size_t tb = a->tmp_bytes;
    YH_HIP(rocprim::radix_sort_pairs(a->tmp, tb, (const u64*)a->key, a->key_b, (const u64*)a->cnt, a->cnt_b, (size_t)n, 0u, bits, st));
    k_acc_heads<<<acc_blocks(n + 1), SG_THREADS, 0, st>>>(a->key_b, n, a->flag, a->cnt_b);
    tb = a->tmp_bytes;
    YH_HIP(rocprim::exclusive_scan(a->tmp, tb, (const u32*)a->flag, a->rank, 0u, (size_t)n + 1, rocprim::plus<u32>(), st));
    tb = a->tmp_bytes;
    YH_HIP(rocprim::exclusive_scan(a->tmp, tb, (const u64*)a->cnt_b, a->pre, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), st));
    k_acc_emit<<<acc_blocks(n), SG_THREADS, 0, st>>>(a->key_b, n, a->flag, a->rank, a->pre, a->key, a->cnt);
    YH_HIP(hipGetLastError());
    u32 distinct = 0;
    YH_HIP(hipMemcpyAsync(&distinct, a->rank + n, sizeof(u32), hipMemcpyDeviceToHost, st));
    YH_HIP(hipStreamSynchronize(st));
    a->n_entries = a->n_compacted = a->n_filled = distinct;
    ++a->n_compactions;
    if (a->capacity - distinct < distinct) YH_TRY(acc_grow(a, std::max<u64>(2ull * distinct, std::min<u64>(2 * a->capacity, ACC_MAX_CAP))));
    return YH_OK;
}

// compacted, with room for `more` entries behind the D distinct ones (and for D, as after every compaction)
static int acc_make_room(yh_sketch_acc* a, u64 more) {
    YH_TRY(acc_compact(a));
    const u64 need = a->n_entries + std::max<u64>(more, a->n_entries);
    if (a->capacity < need) YH_TRY(acc_grow(a, need > ACC_MAX_CAP ? need : std::max<u64>(need, std::min<u64>(2 * a->capacity, ACC_MAX_CAP))));
    return YH_OK;
}

// The chunk's kept hashes behind the log's tail; *total = how many there are (more than the free entries: not all were
// stored).  h_seq: the chunk is on the host and goes up into a->d_seq in pieces under the hashing, as in yh_sketch_dna.
static int acc_hash(yh_sketch_acc* a, const u8* d_seq, const u8* h_seq, u64 n_bytes, u64* total) {
    const u64 n_win = n_bytes - a->k + 1, room = a->capacity - a->n_entries;
    u64* tail = a->key + a->n_entries;
    YH_HIP(hipMemsetAsync(a->d_cnt, 0, sizeof(u64), a->s_comp));
    if (!h_seq) {
        YH_TRY(launch_sketch(d_seq, n_bytes, a->k, a->seed, a->max_hash, room, tail, a->d_cnt, a->s_comp, 0, n_win));
    } else {
        const u64 piece = 32ull << 20;
        u64 done_win = 0;
        int flip = 0;
        for (u64 p0 = 0; p0 < n_bytes; p0 += piece, flip ^= 1) {
            const u64 p1 = std::min<u64>(n_bytes, p0 + piece);
            YH_HIP(hipMemcpyAsync(a->d_seq + p0, h_seq + p0, p1 - p0, hipMemcpyHostToDevice, a->s_copy));
            YH_HIP(hipEventRecord(a->ev[flip], a->s_copy));
            YH_HIP(hipStreamWaitEvent(a->s_comp, a->ev[flip], 0));
            // windows whose bytes are all there, in whole workgroups (the last piece: all that is left)
            const u64 avail = p1 >= a->k ? p1 - a->k + 1 : 0;
            const u64 upto = (p1 == n_bytes) ? n_win : (avail / SK_WIN_ALIGN) * SK_WIN_ALIGN;
            if (upto > done_win) {
                YH_TRY(launch_sketch(a->d_seq, p1, a->k, a->seed, a->max_hash, room, tail, a->d_cnt, a->s_comp, done_win, upto));
                done_win = upto;
            }
        }
    }
    YH_HIP(hipMemcpyAsync(total, a->d_cnt, sizeof(u64), hipMemcpyDeviceToHost, a->s_comp));
    YH_HIP(hipStreamSynchronize(a->s_comp));
    return YH_OK;
}

static int acc_add_chunk(yh_sketch_acc* a, const u8* d_seq, const u8* h_seq, u64 n_bytes) {
    if (n_bytes < a->k) { a->n_bytes += n_bytes; return YH_OK; }
    // a log too full for what this chunk is expected to keep is compacted first: the chunk is then hashed once
    const u64 n_win = n_bytes - a->k + 1;
    const double keep = ((double)a->max_hash + 1.0) / 18446744073709551616.0;
    const u64 expect = std::min<u64>(n_win, (u64)((double)n_win * keep * 1.25) + 4096);
    if (a->capacity - a->n_entries < expect) YH_TRY(acc_compact(a));
    u64 total = 0;
    YH_TRY(acc_hash(a, d_seq, h_seq, n_bytes, &total));
    if (total > a->capacity - a->n_entries) {  // nothing of it counts: room for the reported number, then once more from HBM
        YH_TRY(acc_make_room(a, total));
        ++a->n_rehashed;
        u64 again = 0;
        YH_TRY(acc_hash(a, d_seq, nullptr, n_bytes, &again));
        if (again != total) { yh_set_error("kept hashes changed between two passes"); return YH_ERR_HIP; }
    }
    a->n_entries += total;
    a->n_kept += total;
    a->n_bytes += n_bytes;
    return YH_OK;
}

extern "C" int yh_sketch_acc_create(int device_id, int ksize, uint64_t seed, uint64_t max_hash, uint64_t cap_entries, yh_sketch_acc** out) {
    if (!out) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    *out = nullptr;
    if (ksize < 1 || ksize > 255) { yh_set_error("ksize must be in [1, 255]"); return YH_ERR_INVALID_ARG; }
    if (cap_entries > ACC_MAX_CAP) { yh_set_error("cap_entries must be at most %llu", ACC_MAX_CAP); return YH_ERR_INVALID_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        yh_set_error("no HIP device available (libyacht_hip has no CPU fallback)");
        return YH_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { yh_set_error("device_id %d out of range", device_id); return YH_ERR_NO_DEVICE; }
    YH_HIP(hipSetDevice(device_id));
    yh_sketch_acc* a = new yh_sketch_acc();
    a->device = device_id; a->k = (u32)ksize; a->seed = seed; a->max_hash = max_hash;
    auto init = [&]() -> int {
        YH_HIP(hipStreamCreateWithFlags(&a->s_copy, hipStreamNonBlocking));
        YH_HIP(hipStreamCreateWithFlags(&a->s_comp, hipStreamNonBlocking));
        YH_HIP(hipEventCreateWithFlags(&a->ev[0], hipEventDisableTiming));
        YH_HIP(hipEventCreateWithFlags(&a->ev[1], hipEventDisableTiming));
        YH_HIP(hipMalloc((void**)&a->d_cnt, sizeof(u64)));
        return acc_grow(a, cap_entries ? cap_entries : ACC_DEFAULT_CAP);
    };
    const int rc = init();
    if (rc != YH_OK) { (void)yh_sketch_acc_destroy(a); return rc; }
    *out = a;
    return YH_OK;
}

extern "C" int yh_sketch_acc_destroy(yh_sketch_acc* a) {
    if (!a) return YH_OK;
    if (a->device >= 0) (void)hipSetDevice(a->device);
    if (a->s_copy) { (void)hipStreamSynchronize(a->s_copy); (void)hipStreamDestroy(a->s_copy); }
    if (a->s_comp) { (void)hipStreamSynchronize(a->s_comp); (void)hipStreamDestroy(a->s_comp); }
    for (hipEvent_t e : a->ev) if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)a->key, (void*)a->cnt, (void*)a->work, a->tmp, (void*)a->d_seq, (void*)a->d_cnt}) if (p) (void)hipFree(p);
    delete a;
    return YH_OK;
}

extern "C" int yh_sketch_acc_add(yh_sketch_acc* a, const uint8_t* seq, uint64_t n_bytes) {
    if (!acc_ok(a)) return YH_ERR_INVALID_ARG;
    if (n_bytes && !seq) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    YH_HIP(hipSetDevice(a->device));
    if (n_bytes >= a->k && a->seq_cap < n_bytes) {
        if (a->d_seq) (void)hipFree(a->d_seq);
        a->d_seq = nullptr; a->seq_cap = 0;
        YH_HIP(hipMalloc((void**)&a->d_seq, n_bytes + 64));
        a->seq_cap = n_bytes;
    }
    const int rc = acc_add_chunk(a, a->d_seq, seq, n_bytes);
    if (rc != YH_OK) { (void)hipStreamSynchronize(a->s_copy); (void)hipStreamSynchronize(a->s_comp); }  // (the caller's buffer is let go)
    return rc;
}

extern "C" int yh_sketch_acc_add_device(yh_sketch_acc* a, const uint8_t* d_seq, uint64_t n_bytes) {
    if (!acc_ok(a)) return YH_ERR_INVALID_ARG;
    if (n_bytes && !d_seq) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    YH_HIP(hipSetDevice(a->device));
    const int rc = acc_add_chunk(a, d_seq, nullptr, n_bytes);
    if (rc != YH_OK) (void)hipStreamSynchronize(a->s_comp);
    return rc;
}

extern "C" int yh_sketch_acc_add_hashes(yh_sketch_acc* a, const uint64_t* hashes, const uint64_t* counts, uint64_t n) {
    if (!acc_ok(a)) return YH_ERR_INVALID_ARG;
    if (n && !hashes) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    for (u64 i = 0; i < n; ++i)
        if (hashes[i] > a->max_hash) { yh_set_error("hash %llu (entry %llu) is above max_hash %llu", (u64)hashes[i], i, a->max_hash); return YH_ERR_INVALID_ARG; }
    if (!n) return YH_OK;
    if (n > ACC_MAX_CAP) { yh_set_error("the accumulator holds at most %llu entries", ACC_MAX_CAP); return YH_ERR_UNSUPPORTED; }
    YH_HIP(hipSetDevice(a->device));
    if (a->capacity - a->n_entries < n) YH_TRY(acc_make_room(a, n));
    hipStream_t st = a->s_comp;
    const u64 at = a->n_entries;
    if (a->n_filled < at) k_acc_ones<<<acc_blocks(at - a->n_filled), SG_THREADS, 0, st>>>(a->cnt + a->n_filled, at - a->n_filled);
    if (!counts) k_acc_ones<<<acc_blocks(n), SG_THREADS, 0, st>>>(a->cnt + at, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(a->key + at, hashes, n * sizeof(u64), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && counts) e = hipMemcpyAsync(a->cnt + at, counts, n * sizeof(u64), hipMemcpyHostToDevice, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { yh_set_error("adding hashes failed: %s", hipGetErrorString(e)); return YH_ERR_HIP; }
    a->n_entries = a->n_filled = at + n;
    a->n_kept += n;
    return YH_OK;
}

extern "C" int yh_sketch_acc_get_info(yh_sketch_acc* a, yh_sketch_acc_info* info) {
    if (!acc_ok(a)) return YH_ERR_INVALID_ARG;
    if (!info) { yh_set_error("info is null"); return YH_ERR_INVALID_ARG; }
    info->n_bytes = a->n_bytes;
    info->n_kept = a->n_kept;
    info->n_entries = a->n_entries;
    info->n_compacted = a->n_compacted;
    info->capacity = a->capacity;
    info->n_compactions = a->n_compactions;
    info->n_rehashed_chunks = a->n_rehashed;
    return YH_OK;
}

extern "C" int yh_sketch_acc_finish_device(yh_sketch_acc* a, const uint64_t** d_mins, const uint64_t** d_abund, uint64_t* n) {
    if (!acc_ok(a)) return YH_ERR_INVALID_ARG;
    if (!d_mins || !d_abund || !n) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    YH_HIP(hipSetDevice(a->device));
    YH_TRY(acc_compact(a));
    *d_mins = (const uint64_t*)a->key;
    *d_abund = (const uint64_t*)a->cnt;
    *n = a->n_compacted;
    return YH_OK;
}

extern "C" int yh_sketch_acc_finish(yh_sketch_acc* a, uint64_t cap, uint64_t* mins_out, uint64_t* abund_out, uint64_t* n_out) {
    if (!acc_ok(a)) return YH_ERR_INVALID_ARG;
    if (!n_out || (cap && (!mins_out || !abund_out))) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    *n_out = 0;
    YH_HIP(hipSetDevice(a->device));
    YH_TRY(acc_compact(a));
    const u64 n = a->n_compacted;
    *n_out = n;
    if (!cap || !n) return YH_OK;
    if (n > cap) { yh_set_error("sketch buffers hold %llu entries, %llu needed", (u64)cap, n); return YH_ERR_CAPACITY; }
    YH_HIP(hipMemcpyAsync(mins_out, a->key, n * sizeof(u64), hipMemcpyDeviceToHost, a->s_comp));
    YH_HIP(hipMemcpyAsync(abund_out, a->cnt, n * sizeof(u64), hipMemcpyDeviceToHost, a->s_comp));
    YH_HIP(hipStreamSynchronize(a->s_comp));
    return YH_OK;
}
