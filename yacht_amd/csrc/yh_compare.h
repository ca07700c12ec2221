// yh_compare.h — what the two routes of the compare pass share (yh_compare.hip: the dense tiles; yh_compare_sparse.hip:
// the route through shared hashes): a side's arrays, the self rows, the 128-bit wave sums and the host form's checks and
// uploads.  Everything sits in an unnamed namespace: each of the two files gets its own copy.
#pragma once
#include "yh_common.h"

namespace {

constexpr u32 CMP_THREADS = 256;
constexpr u32 CMP_WAVES = CMP_THREADS / 64;

struct CmpSide {
    const u64* h;      // samples back to back
    const u64* off;    // [n + 1]
    const u32* abund;  // or null: every abundance is 1
    const u8* keep;    // or null: every hash takes part
    u32 n;
};

struct CmpArgs {
    CmpSide a, b;
    u32 keep_and, keep_eq;
    yh_compare_cell* cells;
    u64 ld;
    u64* partial;  // [tiles][n_windows][64][4] when n_windows > 1
    u64* hmax;     // the call's largest hash when n_windows > 1 (cleared in front, k_compare_self raises it), else null
    u32 tiles_b;
    u32 log2_windows;
    u32 symmetric;
};

// a 128-bit sum over the wave: the low words' sum first, its carries counted into the high words
__device__ __forceinline__ void wave_sum128(u64& lo, u64& hi) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o_lo = (u64)__shfl_xor((unsigned long long)lo, d), o_hi = (u64)__shfl_xor((unsigned long long)hi, d);
        lo += o_lo;
        hi += o_hi + (lo < o_lo);
    }
}

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (u64)__shfl_xor((unsigned long long)v, d);
    return v;
}

// the self rows: workgroup s < n_a is A's sample s, the others B's
__global__ void __launch_bounds__(CMP_THREADS) k_compare_self(const CmpArgs q, yh_compare_self* __restrict__ self_a,
                                                               yh_compare_self* __restrict__ self_b) {
    __shared__ u64 s_part[CMP_WAVES][4];
    const bool is_b = blockIdx.x >= q.a.n;
    const CmpSide& sd = is_b ? q.b : q.a;
    const u32 g = is_b ? blockIdx.x - q.a.n : blockIdx.x;
    const u64 lo = sd.off[g], hi = sd.off[g + 1];
    u64 n = 0, sum = 0, sq_lo = 0, sq_hi = 0;
    for (u64 k = lo + threadIdx.x; k < hi; k += CMP_THREADS) {
        if (sd.keep && ((u32)sd.keep[k] & q.keep_and) != q.keep_eq) continue;
        const u64 a = sd.abund ? sd.abund[k] : 1u;
        const u64 p = a * a;
        n += 1;
        sum += a;
        sq_lo += p;
        sq_hi += (sq_lo < p);
    }
    n = wave_sum64(n);
    sum = wave_sum64(sum);
    wave_sum128(sq_lo, sq_hi);
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) s_part[wave][0] = n, s_part[wave][1] = sum, s_part[wave][2] = sq_lo, s_part[wave][3] = sq_hi;
    __syncthreads();
    if (threadIdx.x != 0) return;
    yh_compare_self r{0, 0, 0, 0};
    for (u32 v = 0; v < CMP_WAVES; ++v) {
        r.n_kept += s_part[v][0];
        r.sum += s_part[v][1];
        r.sq_lo += s_part[v][2];
        r.sq_hi += s_part[v][3] + (r.sq_lo < s_part[v][2]);
    }
    (is_b ? self_b : self_a)[g] = r;
    if (q.hmax && hi > lo) atomicMax(q.hmax, sd.h[hi - 1]);  // (a sample's last hash is its largest)
}

bool same_side(const void* a, const void* ao, const void* aa, const void* ak, u64 na, u64 ta, const void* b, const void* bo,
               const void* ba, const void* bk, u64 nb, u64 tb) {
    return a == b && ao == bo && aa == ba && ak == bk && na == nb && ta == tb;
}

int compare_args_ok(u64 n_a, u64 n_b, u64 ld_cells) {
    if (n_a > YH_COMPARE_MAX_SAMPLES || n_b > YH_COMPARE_MAX_SAMPLES) {
        yh_set_error("yh_compare takes at most %d samples a side, not %llu x %llu", YH_COMPARE_MAX_SAMPLES, (u64)n_a, (u64)n_b);
        return YH_ERR_INVALID_ARG;
    }
    if (ld_cells < n_b) { yh_set_error("ld_cells %llu is smaller than n_b %llu", (u64)ld_cells, (u64)n_b); return YH_ERR_INVALID_ARG; }
    return YH_OK;
}

// the host form's checks of one side: offsets from 0, never descending, a sample shorter than 2^32, hashes strictly ascending
int compare_check_side(const char* name, const uint64_t* h, const uint64_t* off, uint64_t n) {
    if (n == 0) return YH_OK;
    if (!off) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    if (off[0] != 0) { yh_set_error("offsets of %s must start at 0", name); return YH_ERR_INVALID_ARG; }
    for (u64 s = 0; s < n; ++s) {
        if (off[s] > off[s + 1]) { yh_set_error("offsets of %s descend at sample %llu", name, s); return YH_ERR_INVALID_ARG; }
        if (off[s + 1] - off[s] >= (1ull << 32)) { yh_set_error("sample %llu of %s has 2^32 hashes or more", s, name); return YH_ERR_INVALID_ARG; }
    }
    if (off[n] && !h) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    for (u64 s = 0; s < n; ++s)
        for (u64 k = off[s] + 1; k < off[s + 1]; ++k)
            if (h[k - 1] >= h[k]) { yh_set_error("sample %llu of %s is not strictly ascending at entry %llu", s, name, k - off[s]); return YH_ERR_UNSORTED; }
    return YH_OK;
}

struct CmpDevSide {
    uint64_t* h = nullptr;
    uint64_t* off = nullptr;
    uint32_t* abund = nullptr;
    uint8_t* keep = nullptr;
    yh_compare_self* self = nullptr;
    void release() {
        (void)hipFree(h); (void)hipFree(off); (void)hipFree(abund); (void)hipFree(keep); (void)hipFree(self);
    }
};

int compare_upload(CmpDevSide& d, const uint64_t* h, const uint64_t* off, const uint32_t* abund, const uint8_t* keep, u64 n) {
    const u64 total = off[n];
    YH_HIP(hipMalloc((void**)&d.off, (n + 1) * sizeof(u64)));
    YH_HIP(hipMemcpy(d.off, off, (n + 1) * sizeof(u64), hipMemcpyHostToDevice));
    YH_HIP(hipMalloc((void**)&d.self, n * sizeof(yh_compare_self)));
    if (total) {
        YH_HIP(hipMalloc((void**)&d.h, total * sizeof(u64)));
        YH_HIP(hipMemcpy(d.h, h, total * sizeof(u64), hipMemcpyHostToDevice));
        if (abund) {
            YH_HIP(hipMalloc((void**)&d.abund, total * sizeof(u32)));
            YH_HIP(hipMemcpy(d.abund, abund, total * sizeof(u32), hipMemcpyHostToDevice));
        }
        if (keep) {
            YH_HIP(hipMalloc((void**)&d.keep, total));
            YH_HIP(hipMemcpy(d.keep, keep, total, hipMemcpyHostToDevice));
        }
    }
    return YH_OK;
}

}  // namespace
