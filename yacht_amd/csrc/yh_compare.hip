// yh_compare.hip — sample against sample: for every pair of sorted sketches the size of the intersection, the sum of the
// smaller abundances and the 128-bit sum of their products (yh_compare_device, include/yacht_hip.h).  No yh_db.
//
// Every other pass measures samples against the database through its directory.  Samples from one environment share
// most hashes with hundreds of others: posting lists would be as long as the cohort.  This is a dense S x S pass over the
// sorted arrays themselves, with abundances on both sides.
//
// k_compare_tiles.  A workgroup OWNS a tile of CMP_TILE x CMP_TILE cells and one window of the hash space: one of
// n_windows equal parts of [0, the call's largest hash] (k_compare_self leaves that maximum in the work memory: a sketch of
// scaled = 1000 fills a thousandth of the 64-bit range).  Hashes are uniform, so the windows hold equal parts of every
// sample.  It walks the window in rounds.  A round stages the next CMP_SLICE entries of each of the tile's 16 samples in LDS -- hash, abundance, keep bit --
// read once from HBM, coalesced, and reused by all 64 cells.  The round's bound H is the smallest LAST staged hash among the
// samples that have more to come: up to H every sample's entries are complete in LDS, so the cells may be merged up to H,
// and every sample moves on by its entries <= H.  The sample that set H moves on by a full slice, so the walk ends; a
// slice is never truncated, whatever the distribution (clustered hashes, a narrow range, one long and fifteen short
// samples only cost rounds).  Uniform samples of similar size all move on by nearly a slice per round.
//   A LANE OWNS A CELL: lane l of each of the four waves merges A sample (l & 7) with B sample (l >> 3), two cursors into
// LDS, 8-byte reads, its four sums in registers.  The waves split a round by quarters of A's entries; wave v finds its
// place in B by one binary search.  No atomics anywhere, no clearing pass: the four waves' sums meet once, in LDS, when the
// window is done, carries taken from the low words' sums.  Each cell is written exactly once -- to the matrix when there
// is one window, else to the tile's partial slab in the work memory, which k_compare_reduce sums in a fixed order.
//   Small cohorts have few tiles: the host cuts the hash space into up to YH_COMPARE_MAX_WINDOWS windows until the grid
// fills the device.  The symmetric call (the same pointers for A and B) runs only the tiles with i-tile <= j-tile and
// writes their mirror images.
//
// k_compare_self.  One workgroup per sample of A and of B: kept hashes, sum and 128-bit sum of squares.
//
// Three launches at most, whatever the number of samples.  All sums are integers: the result does not depend on the order
// anything ran in.
#include "yh_compare.h"

#include <algorithm>
#include <vector>

namespace {

constexpr u32 CMP_TILE = YH_COMPARE_TILE;
constexpr u32 CMP_SLICE = YH_COMPARE_SLICE;
constexpr u32 CMP_NS = 2 * CMP_TILE;           // samples a tile stages: its A samples, then its B samples
constexpr u32 CMP_CELLS = CMP_TILE * CMP_TILE;
constexpr u32 CMP_ROW = CMP_SLICE + 1;         // a staged row in 8-byte words: one word of padding, so that equal positions of the rows fall on different banks
static_assert(CMP_CELLS == 64, "a lane of a wave owns a cell");
static_assert(CMP_SLICE == CMP_THREADS, "a thread stages one entry per sample and round");
static_assert(CMP_NS * CMP_ROW >= CMP_WAVES * CMP_CELLS * 4, "the waves' sums reuse the staged hashes");

// (CmpSide, CmpArgs, k_compare_self and the wave sums: yh_compare.h, shared with the sparse route)
__device__ __forceinline__ u64 lower_bound_global(const u64* __restrict__ p, u64 lo, u64 hi, u64 v) {
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (p[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(CMP_THREADS) k_compare_tiles(const CmpArgs q) {
    __shared__ u64 s_h[CMP_NS * CMP_ROW];
    __shared__ u32 s_ab[CMP_NS * CMP_SLICE];
    __shared__ u8 s_kp[CMP_NS * CMP_SLICE];
    __shared__ u64 s_cur[CMP_NS], s_end[CMP_NS];
    __shared__ u32 s_cnt[CMP_NS], s_adv[CMP_NS];
    __shared__ u64 s_bound;

    const u32 ti = blockIdx.x / q.tiles_b, tj = blockIdx.x % q.tiles_b;
    if (q.symmetric && ti > tj) return;  // (the mirror image of tile (tj, ti))
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 n_windows = 1u << q.log2_windows, w = blockIdx.y;

    if (tid < CMP_NS) {  // this sample's part of the window: [cur, end) in its side's arrays
        const bool is_b = tid >= CMP_TILE;
        const CmpSide& sd = is_b ? q.b : q.a;
        const u32 g = (is_b ? tj : ti) * CMP_TILE + (tid & (CMP_TILE - 1));
        u64 cur = 0, end = 0;
        if (g < sd.n) {
            const u64 lo = sd.off[g], hi = sd.off[g + 1];
            cur = lo, end = hi;
            if (q.log2_windows) {  // window w is [w * step, (w + 1) * step), the last one open: (n_windows - 1) * step < 2^64
                const u64 step = (*q.hmax >> q.log2_windows) + 1;
                if (w) cur = lower_bound_global(sd.h, lo, hi, (u64)w * step);
                if (w + 1 < n_windows) end = lower_bound_global(sd.h, cur, hi, (u64)(w + 1) * step);
            }
        }
        s_cur[tid] = cur;
        s_end[tid] = end;
    }
    if (tid == 0) s_bound = ~0ull;
    __syncthreads();

    const u32 ia = lane & (CMP_TILE - 1), jb = CMP_TILE + (lane >> 3);  // this lane's cell: staged rows ia and jb
    const u64* __restrict__ ha = s_h + ia * CMP_ROW;
    const u64* __restrict__ hb = s_h + jb * CMP_ROW;
    u64 c_n = 0, c_min = 0, c_lo = 0, c_hi = 0;

    for (;;) {
        bool a_left = false, b_left = false;
#pragma unroll
        for (u32 s = 0; s < CMP_TILE; ++s) {
            a_left |= s_cur[s] < s_end[s];
            b_left |= s_cur[CMP_TILE + s] < s_end[CMP_TILE + s];
        }
        if (!(a_left && b_left)) break;  // (workgroup-uniform: nothing left that could be shared)
        // stage: thread e takes entry e of every sample's next slice
#pragma unroll 4
        for (u32 s = 0; s < CMP_NS; ++s) {
            const CmpSide& sd = s >= CMP_TILE ? q.b : q.a;
            const u64 cur = s_cur[s], left = s_end[s] - cur;
            if ((u64)tid < left) {
                const u64 at = cur + tid;
                s_h[s * CMP_ROW + tid] = sd.h[at];
                s_ab[s * CMP_SLICE + tid] = sd.abund ? sd.abund[at] : 1u;
                s_kp[s * CMP_SLICE + tid] = sd.keep ? (u8)(((u32)sd.keep[at] & q.keep_and) == q.keep_eq) : (u8)1;
            }
        }
        __syncthreads();
        if (tid < CMP_NS) {  // the bound: the smallest last staged hash of a sample that has more behind its slice
            const u64 left = s_end[tid] - s_cur[tid];
            s_cnt[tid] = (u32)min(left, (u64)CMP_SLICE);
            if (left > CMP_SLICE) atomicMin(&s_bound, s_h[tid * CMP_ROW + CMP_SLICE - 1]);
        }
        __syncthreads();
        const u64 bound = s_bound;
        if (tid < CMP_NS) {  // entries <= bound of this sample's slice (upper bound)
            const u64* __restrict__ row = s_h + tid * CMP_ROW;
            u32 lo = 0, hi = s_cnt[tid];
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (row[mid] <= bound) lo = mid + 1; else hi = mid;
            }
            s_adv[tid] = lo;
        }
        __syncthreads();
        {   // merge this cell's quarter of the round
            const u32 na = s_adv[ia], nb = s_adv[jb];
            u32 pa = (u32)((u64)na * wave / CMP_WAVES);
            const u32 ea = (u32)((u64)na * (wave + 1) / CMP_WAVES);
            u32 pb = 0;
            if (pa < ea && pa > 0) {  // B's first entry >= this quarter's first A entry
                const u64 v = ha[pa];
                u32 hi = nb;
                while (pb < hi) {
                    const u32 mid = (pb + hi) >> 1;
                    if (hb[mid] < v) pb = mid + 1; else hi = mid;
                }
            }
            while (pa < ea && pb < nb) {
                const u64 x = ha[pa], y = hb[pb];
                if (x == y) {
                    if (s_kp[ia * CMP_SLICE + pa] & s_kp[jb * CMP_SLICE + pb]) {
                        const u32 u = s_ab[ia * CMP_SLICE + pa], v = s_ab[jb * CMP_SLICE + pb];
                        const u64 p = (u64)u * (u64)v;
                        c_n += 1;
                        c_min += min(u, v);
                        c_lo += p;
                        c_hi += (c_lo < p);
                    }
                }
                pa += (x <= y);
                pb += (y <= x);
            }
        }
        __syncthreads();
        if (tid < CMP_NS) s_cur[tid] += s_adv[tid];
        if (tid == 0) s_bound = ~0ull;
        __syncthreads();
    }

    // the four waves' sums of the 64 cells meet in LDS (the staged hashes are done with), wave 0 adds them up
    __syncthreads();
    u64* red = s_h;
    red[(wave * CMP_CELLS + lane) * 4 + 0] = c_n;
    red[(wave * CMP_CELLS + lane) * 4 + 1] = c_min;
    red[(wave * CMP_CELLS + lane) * 4 + 2] = c_lo;
    red[(wave * CMP_CELLS + lane) * 4 + 3] = c_hi;
    __syncthreads();
    if (wave != 0) return;
    u64 t_n = 0, t_min = 0, t_lo = 0, t_hi = 0;
#pragma unroll
    for (u32 v = 0; v < CMP_WAVES; ++v) {
        const u64* r = red + (v * CMP_CELLS + lane) * 4;
        t_n += r[0];
        t_min += r[1];
        t_lo += r[2];
        t_hi += r[3] + (t_lo < r[2]);
    }
    if (q.log2_windows) {
        u64* out = q.partial + (((u64)blockIdx.x << q.log2_windows) + w) * (CMP_CELLS * 4) + lane * 4;
        out[0] = t_n, out[1] = t_min, out[2] = t_lo, out[3] = t_hi;
        return;
    }
    const u32 gi = ti * CMP_TILE + ia, gj = tj * CMP_TILE + (lane >> 3);
    if (gi < q.a.n && gj < q.b.n) {
        const yh_compare_cell c{t_n, t_min, t_lo, t_hi};
        q.cells[(u64)gi * q.ld + gj] = c;
        if (q.symmetric && ti != tj) q.cells[(u64)gj * q.ld + gi] = c;
    }
}

// cells from the windows' partial slabs: one thread per cell of a tile, the windows in ascending order
__global__ void __launch_bounds__(256) k_compare_reduce(const CmpArgs q, u32 n_tiles) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    const u32 tile = (u32)(t / CMP_CELLS), lane = (u32)(t % CMP_CELLS);
    if (tile >= n_tiles) return;
    const u32 ti = tile / q.tiles_b, tj = tile % q.tiles_b;
    if (q.symmetric && ti > tj) return;
    const u32 gi = ti * CMP_TILE + (lane & (CMP_TILE - 1)), gj = tj * CMP_TILE + (lane >> 3);
    if (gi >= q.a.n || gj >= q.b.n) return;
    u64 t_n = 0, t_min = 0, t_lo = 0, t_hi = 0;
    const u64* __restrict__ p = q.partial + ((u64)tile << q.log2_windows) * (CMP_CELLS * 4) + lane * 4;
    for (u32 w = 0; w < (1u << q.log2_windows); ++w, p += CMP_CELLS * 4) {
        t_n += p[0];
        t_min += p[1];
        t_lo += p[2];
        t_hi += p[3] + (t_lo < p[2]);
    }
    const yh_compare_cell c{t_n, t_min, t_lo, t_hi};
    q.cells[(u64)gi * q.ld + gj] = c;
    if (q.symmetric && ti != tj) q.cells[(u64)gj * q.ld + gi] = c;
}

// How a call is cut: the tiles, and how many windows of the hash space each tile is split into so that the grid fills
// the device.  A window should still hold a few slices of an average sample, or the rounds are mostly staging.
struct CmpPlan {
    u32 tiles_a, tiles_b, log2_windows;
    u64 partial_bytes;
};

CmpPlan compare_plan(u64 n_a, u64 n_b, u64 total_a, u64 total_b, bool symmetric) {
    CmpPlan p{};
    p.tiles_a = (u32)((n_a + CMP_TILE - 1) / CMP_TILE);
    p.tiles_b = (u32)((n_b + CMP_TILE - 1) / CMP_TILE);
    const u64 tiles = (u64)p.tiles_a * p.tiles_b;
    const u64 active = symmetric ? (u64)p.tiles_a * (p.tiles_a + 1) / 2 : tiles;
    u32 lg = 0;
    if (active) {
        const u64 avg = (n_a ? total_a / n_a : 0) + (n_b ? total_b / n_b : 0);  // entries of an average cell
        while ((1u << lg) < YH_COMPARE_MAX_WINDOWS && (active << lg) < 1024 && (avg >> (lg + 1)) >= 4ull * CMP_SLICE) ++lg;
    }
    p.log2_windows = lg;
    p.partial_bytes = lg ? 256 + (tiles << lg) * (CMP_CELLS * 4 * sizeof(u64)) : 0;  // (the largest hash in front)
    return p;
}

}  // namespace

extern "C" uint64_t yh_compare_work_bytes(uint64_t n_a, uint64_t n_b, uint64_t total_a, uint64_t total_b) {
    if (n_a > YH_COMPARE_MAX_SAMPLES || n_b > YH_COMPARE_MAX_SAMPLES) return 0;
    // (the symmetric call runs fewer tiles and may cut them into more windows: room for whichever the pointers turn out to ask for)
    return std::max(compare_plan(n_a, n_b, total_a, total_b, false).partial_bytes,
                    compare_plan(n_a, n_b, total_a, total_b, true).partial_bytes) + 256;
}

extern "C" int yh_compare_device(const uint64_t* d_a, const uint64_t* d_a_off, const uint32_t* d_a_abund, const uint8_t* d_a_keep,
                                 uint64_t n_a, uint64_t total_a, const uint64_t* d_b, const uint64_t* d_b_off,
                                 const uint32_t* d_b_abund, const uint8_t* d_b_keep, uint64_t n_b, uint64_t total_b, uint8_t keep_and,
                                 uint8_t keep_eq, yh_compare_cell* d_cells, uint64_t ld_cells, yh_compare_self* d_self_a,
                                 yh_compare_self* d_self_b, void* d_work, uint64_t work_bytes, void* stream) {
    YH_TRY(compare_args_ok(n_a, n_b, ld_cells));
    if ((n_a && (!d_a_off || !d_self_a)) || (n_b && (!d_b_off || !d_self_b)) || (n_a && n_b && !d_cells) || (total_a && !d_a) ||
        (total_b && !d_b)) {
        yh_set_error("null argument");
        return YH_ERR_INVALID_ARG;
    }
    if (n_a + n_b == 0) return YH_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool sym = same_side(d_a, d_a_off, d_a_abund, d_a_keep, n_a, total_a, d_b, d_b_off, d_b_abund, d_b_keep, n_b, total_b);
    const CmpPlan p = compare_plan(n_a, n_b, total_a, total_b, sym);
    u64* partial = nullptr;
    if (p.partial_bytes) {
        if (!d_work || work_bytes < p.partial_bytes + 256) {
            yh_set_error("work buffer holds %llu bytes, %llu needed", (u64)work_bytes, (u64)(p.partial_bytes + 256));
            return YH_ERR_INVALID_ARG;
        }
        partial = reinterpret_cast<u64*>((reinterpret_cast<uintptr_t>(d_work) + 255u) & ~(uintptr_t)255u);
        YH_HIP(hipMemsetAsync(partial, 0, sizeof(u64), st));
    }
    CmpArgs q{};
    q.a = CmpSide{(const u64*)d_a, (const u64*)d_a_off, d_a_abund, d_a_keep, (u32)n_a};
    q.b = CmpSide{(const u64*)d_b, (const u64*)d_b_off, d_b_abund, d_b_keep, (u32)n_b};
    q.keep_and = keep_and, q.keep_eq = keep_eq;
    q.cells = d_cells, q.ld = ld_cells, q.partial = partial ? partial + 32 : nullptr, q.hmax = partial;
    q.tiles_b = p.tiles_b, q.log2_windows = p.log2_windows, q.symmetric = sym ? 1u : 0u;
    k_compare_self<<<(u32)(n_a + n_b), CMP_THREADS, 0, st>>>(q, d_self_a, d_self_b);
    const u32 n_tiles = p.tiles_a * p.tiles_b;
    if (n_tiles) {
        k_compare_tiles<<<dim3(n_tiles, 1u << p.log2_windows), CMP_THREADS, 0, st>>>(q);
        if (p.log2_windows) k_compare_reduce<<<(u32)(((u64)n_tiles * CMP_CELLS + 255) / 256), 256, 0, st>>>(q, n_tiles);
    }
    if (hipGetLastError() != hipSuccess) { yh_set_error("compare launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

extern "C" int yh_compare(const uint64_t* a, const uint64_t* a_off, const uint32_t* a_abund, const uint8_t* a_keep, uint64_t n_a,
                          const uint64_t* b, const uint64_t* b_off, const uint32_t* b_abund, const uint8_t* b_keep, uint64_t n_b,
                          uint8_t keep_and, uint8_t keep_eq, int device_id, yh_compare_cell* cells, uint64_t ld_cells,
                          yh_compare_self* self_a, yh_compare_self* self_b) {
    YH_TRY(compare_args_ok(n_a, n_b, ld_cells));
    if ((n_a && !self_a) || (n_b && !self_b) || (n_a && n_b && !cells)) { yh_set_error("null argument"); return YH_ERR_INVALID_ARG; }
    YH_TRY(compare_check_side("A", a, a_off, n_a));
    const bool sym = same_side(a, a_off, a_abund, a_keep, n_a, 0, b, b_off, b_abund, b_keep, n_b, 0);
    if (!sym) YH_TRY(compare_check_side("B", b, b_off, n_b));
    if (n_a + n_b == 0) return YH_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        yh_set_error("no HIP device available (libyacht_hip has no CPU fallback)");
        return YH_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { yh_set_error("device_id %d out of range", device_id); return YH_ERR_NO_DEVICE; }
    YH_HIP(hipSetDevice(device_id));
    static const uint64_t zero_off[1] = {0};
    if (n_a == 0) a_off = zero_off;
    if (n_b == 0) b_off = zero_off;
    CmpDevSide da, db;
    yh_compare_cell* d_cells = nullptr;
    void* d_work = nullptr;
    auto run = [&]() -> int {
        YH_TRY(compare_upload(da, a, a_off, a_abund, a_keep, n_a));
        if (!sym) YH_TRY(compare_upload(db, b, b_off, b_abund, b_keep, n_b));
        const CmpDevSide& rb = sym ? da : db;
        const u64 total_a = a_off[n_a], total_b = b_off[n_b];
        const u64 wb = yh_compare_work_bytes(n_a, n_b, total_a, total_b);
        YH_HIP(hipMalloc(&d_work, wb));
        if (n_a && n_b) YH_HIP(hipMalloc((void**)&d_cells, n_a * n_b * sizeof(yh_compare_cell)));
        YH_TRY(yh_compare_device(da.h, da.off, da.abund, da.keep, n_a, total_a, rb.h, rb.off, rb.abund, rb.keep, n_b, total_b, keep_and,
                                 keep_eq, d_cells, n_b, da.self, rb.self, d_work, wb, nullptr));
        YH_HIP(hipDeviceSynchronize());
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
    (void)hipFree(d_work);
    return rc;
}
