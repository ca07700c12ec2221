// yh_matrix.hip — the organism x sample tables of a cohort from what its blocks leave on the device (include/yacht_hip.h:
// yh_matrix_cells_device, yh_matrix_prevalence_device, yh_matrix_fill_device).
//
// A block of a cohort run ends with its compact rows (yh_batch_row, in (reference, sample) order), the present bytes the
// presence test left beside them, one plane per coverage, and with --abundance the median depth gathered at the rows.  The
// first pass turns the rows some coverage calls present into CELLS of 24 bytes: (sample, reference, n_match, a mask with one
// bit per coverage, twice the median depth as an integer).  A cohort's cells stay on the device, block behind block.  After
// the last block the second pass counts, per coverage, the samples every reference is present in and the sum of the depths of
// every sample's present references; the host picks the references to keep from the counts, and the third pass stores every
// kept cell into the wide matrices of one coverage.  All sums are integer sums and no position depends on an atomic, so two
// runs give the same bytes.
#include "yh_matrix.h"

#include <algorithm>

namespace {

// ---- rows -> cells: a stable compaction in three launches (yh_lca.hip's rows pack has the same shape) ------------------------
// The masks of every chunk of YH_MATRIX_CHUNK rows are made and their non-zero ones counted, the chunk counts are scanned by ONE
// workgroup into each chunk's first cell and the total, then every chunk's cells are written behind its first: a row's cell is
// the chunk's first + the cells of the chunk's earlier rounds and waves + those of the lower lanes of its wave (ballots).
constexpr u32 MC_THREADS = 256;
constexpr u32 MC_ROUNDS = YH_MATRIX_CHUNK / MC_THREADS;
constexpr u32 MC_SCAN_THREADS = 1024;
static_assert(YH_MATRIX_CHUNK % MC_THREADS == 0 && MC_ROUNDS >= 1, "a chunk is whole rounds of the workgroup");

__global__ void __launch_bounds__(MC_THREADS) k_matrix_cells_count(const yh_batch_row* __restrict__ rows, const u32* __restrict__ n_rows,
                                                                   u64 cap_rows, const u8* __restrict__ present, u32 n_sets, u64 n_refs,
                                                                   u32* __restrict__ mask, u64* __restrict__ chunk) {
    __shared__ u32 wcnt[MC_THREADS / 64];
    const u64 n = min((u64)*n_rows, cap_rows);
    u32 cnt = 0;
#pragma unroll
    for (u32 r = 0; r < MC_ROUNDS; ++r) {
        const u64 k = blockIdx.x * (u64)YH_MATRIX_CHUNK + r * MC_THREADS + threadIdx.x;
        u32 m = 0;
        if (k < n && rows[k].ref < n_refs)
            for (u32 c = 0; c < n_sets; ++c) m |= (u32)(present[(u64)c * cap_rows + k] != 0) << c;
        if (k < cap_rows) mask[k] = m;
        cnt += (u32)__popcll(__ballot(m != 0));
    }
    if ((threadIdx.x & 63u) == 0) wcnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 total = 0;
        for (u32 w = 0; w < MC_THREADS / 64; ++w) total += wcnt[w];
        chunk[blockIdx.x] = total;
    }
}

// chunk[b] = the cells of the chunks before b; *n_cells = all of them.  One workgroup; n_chunks may be 0.
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_matrix_cells_scan(u64* __restrict__ chunk, u64 n_chunks, u64* __restrict__ n_cells) {
    __shared__ u64 part[MC_SCAN_THREADS];
    const u64 per = (n_chunks + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const u64 lo = min((u64)threadIdx.x * per, n_chunks), hi = min(lo + per, n_chunks);
    u64 mine = 0;
    for (u64 b = lo; b < hi; ++b) mine += chunk[b];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (u32 d = 1; d < MC_SCAN_THREADS; d <<= 1) {  // (inclusive, in place: read, barrier, add, barrier)
        const u64 below = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += below;
        __syncthreads();
    }
    u64 run = part[threadIdx.x] - mine;
    for (u64 b = lo; b < hi; ++b) {
        const u64 c = chunk[b];
        chunk[b] = run;
        run += c;
    }
    if (threadIdx.x == MC_SCAN_THREADS - 1) *n_cells = part[threadIdx.x];
}

__global__ void __launch_bounds__(MC_THREADS) k_matrix_cells_emit(const yh_batch_row* __restrict__ rows, u64 cap_rows,
                                                                  const u32* __restrict__ mask, const double* __restrict__ med,
                                                                  u32 sample_base, const u64* __restrict__ chunk,
                                                                  yh_matrix_cell* __restrict__ cells) {
    __shared__ u32 wcnt[MC_ROUNDS * (MC_THREADS / 64)];
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const u64 first = chunk[blockIdx.x];
    u32 m[MC_ROUNDS];
    u64 bal[MC_ROUNDS];
#pragma unroll
    for (u32 r = 0; r < MC_ROUNDS; ++r) {
        const u64 k = blockIdx.x * (u64)YH_MATRIX_CHUNK + r * MC_THREADS + threadIdx.x;
        m[r] = k < cap_rows ? mask[k] : 0u;
        bal[r] = __ballot(m[r] != 0);
        if (lane == 0) wcnt[r * (MC_THREADS / 64) + wv] = (u32)__popcll(bal[r]);
    }
    __syncthreads();
#pragma unroll
    for (u32 r = 0; r < MC_ROUNDS; ++r) {
        if (m[r] == 0) continue;
        u32 below = 0;
        for (u32 w = 0; w < r * (MC_THREADS / 64) + wv; ++w) below += wcnt[w];
        const u64 at = first + below + (u64)__popcll(bal[r] & ((1ull << lane) - 1ull));
        if (at >= cap_rows) continue;  // (cannot happen: at most one cell per row; kept as the store's bound)
        const u64 k = blockIdx.x * (u64)YH_MATRIX_CHUNK + r * MC_THREADS + threadIdx.x;
        const yh_batch_row row = rows[k];
        yh_matrix_cell cell;
        cell.sample = row.sample + sample_base;
        cell.ref = row.ref;
        cell.n_match = row.n_match;
        cell.mask = m[r];
        const double twice = med ? 2.0 * med[k] : 0.0;  // (x.0 or x.5 doubled: an exact integer; NaN compares false)
        cell.depth2 = twice > 0.0 ? (u64)twice : 0ull;
        cells[at] = cell;
    }
}

// ---- cells -> prevalence counts and per-sample depth sums ---------------------------------------------------------------------
// A workgroup takes PV_TILE consecutive cells.  Prevalence: the cells of one reference lie in a run, so inside a wave the
// lanes of a run are one segment; per coverage one ballot gives every segment's count and the segment's first lane adds it
// with ONE global atomic.  Depth sums: seen by sample the cells are scattered, so a workgroup sums them in an LDS table keyed by
// sample (open addressing, one slot = the sample and one 64-bit sum per coverage) and adds every non-zero sum once when the
// tile is done; a cell that finds no slot within PV_PROBES adds to global memory itself.  Integer atomics only.
constexpr u32 PV_THREADS = 256;
constexpr u32 PV_TILE = YH_MATRIX_TILE;
constexpr u32 PV_ROUNDS = PV_TILE / PV_THREADS;
static_assert(YH_MATRIX_TILE % PV_THREADS == 0 && PV_ROUNDS >= 1, "a tile is whole rounds of the workgroup");
constexpr u32 PV_PROBES = 8;
constexpr u32 PV_EMPTY = 0xffffffffu;
constexpr u32 PV_LDS_BYTES = 48u * 1024u;
constexpr u32 PV_MAX_SLOTS_LOG2 = 11;

__global__ void __launch_bounds__(PV_THREADS) k_matrix_prevalence(const yh_matrix_cell* __restrict__ cells, u64 n_cells, u32 n_sets,
                                                                  u32 n_samples, const u8* __restrict__ skip, u64 n_refs,
                                                                  u32* __restrict__ prev, u64* __restrict__ denom, u32 slots_log2) {
    extern __shared__ u64 pv_lds[];
    const u32 slots = 1u << slots_log2;
    u64* const vals = pv_lds;                                // [slots][n_sets]
    u32* const keys = (u32*)(pv_lds + (u64)slots * n_sets);  // [slots]
    for (u32 i = threadIdx.x; i < slots; i += PV_THREADS) keys[i] = PV_EMPTY;
    for (u32 i = threadIdx.x; i < slots * n_sets; i += PV_THREADS) vals[i] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63u;
    const u32 set_mask = n_sets >= 32 ? 0xffffffffu : (1u << n_sets) - 1u;
    for (u32 r = 0; r < PV_ROUNDS; ++r) {
        const u64 k = blockIdx.x * (u64)PV_TILE + r * PV_THREADS + threadIdx.x;
        u32 ref = PV_EMPTY, smp = 0, m = 0;
        u64 d2 = 0;
        if (k < n_cells) {
            const yh_matrix_cell cell = cells[k];
            if (cell.sample < n_samples && cell.ref < n_refs && !(skip && skip[cell.sample])) {
                ref = cell.ref; smp = cell.sample; m = cell.mask & set_mask; d2 = cell.depth2;
            }
        }
        // the segment of this lane's run inside the wave: [lane, the next lane that starts a run)
        const u32 before = __shfl_up(ref, 1);
        const bool head = lane == 0 || before != ref;
        const u64 heads = __ballot(head);
        const u64 above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
        const u32 end = above ? (u32)__ffsll(above) - 1u : 64u;
        const u64 seg = (end >= 64 ? ~0ull : (1ull << end) - 1ull) & (~0ull << lane);
        for (u32 c = 0; c < n_sets; ++c) {
            const u64 bal = __ballot((m >> c) & 1u);
            if (bal == 0) continue;  // (uniform)
            const u32 cnt = (u32)__popcll(bal & seg);
            if (head && cnt != 0 && ref < n_refs) atomicAdd(&prev[(u64)c * n_refs + ref], cnt);
        }
        if (m != 0 && d2 != 0) {
            u32 slot = (smp * 2654435761u) >> (32 - slots_log2);
            bool placed = false;
            for (u32 p = 0; p < PV_PROBES && !placed; ++p) {
                const u32 s = (slot + p) & (slots - 1);
                const u32 old = atomicCAS(&keys[s], PV_EMPTY, smp);
                if (old == PV_EMPTY || old == smp) { placed = true; slot = s; }
            }
            for (u32 c = 0; c < n_sets; ++c) {
                if (!((m >> c) & 1u)) continue;
                if (placed) atomicAdd(&vals[(u64)slot * n_sets + c], d2);
                else atomicAdd(&denom[(u64)c * n_samples + smp], d2);
            }
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < slots * n_sets; i += PV_THREADS) {
        const u64 v = vals[i];
        if (v == 0) continue;
        const u32 smp = keys[i / n_sets];
        if (smp < n_samples) atomicAdd(&denom[(u64)(i % n_sets) * n_samples + smp], v);
    }
}

// ---- cells -> the wide matrices of one coverage --------------------------------------------------------------------------------
// A (sample, reference) pair has at most one cell, so every cell owns its place in the matrices: plain stores.
__global__ void __launch_bounds__(256) k_matrix_fill(const yh_matrix_cell* __restrict__ cells, u64 n_cells, u32 bit, u32 n_samples,
                                                     const u8* __restrict__ skip, u64 n_refs, const int32_t* __restrict__ row_of_ref,
                                                     u64 n_kept, const u64* __restrict__ denom_bit, u8* __restrict__ presence,
                                                     u32* __restrict__ n_match, double* __restrict__ rel) {
    for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < n_cells; k += (u64)gridDim.x * blockDim.x) {
        const yh_matrix_cell cell = cells[k];
        if (!((cell.mask >> bit) & 1u) || cell.sample >= n_samples || cell.ref >= n_refs) continue;
        if (skip && skip[cell.sample]) continue;
        const int32_t row = row_of_ref[cell.ref];
        if (row < 0 || (u64)row >= n_kept) continue;
        const u64 at = (u64)row * n_samples + cell.sample;
        presence[at] = 1;
        n_match[at] = cell.n_match;
        if (rel) {
            const u64 den = denom_bit[cell.sample];
            rel[at] = den ? (double)cell.depth2 / (double)den : 0.0;
        }
    }
}

}  // namespace

int yh_q_matrix_cells(yh_db* db, const yh_batch_row* d_rows, const u32* d_n_rows, u64 cap_rows, const u8* d_present, u32 n_sets,
                      const double* d_med, u32 sample_base, yh_matrix_cell* d_cells, u64* d_n_cells) {
    hipStream_t st = db->stream;
    const u64 n_chunks = (cap_rows + YH_MATRIX_CHUNK - 1) / YH_MATRIX_CHUNK;
    u64* d_chunk = nullptr;  // the chunks' counts, then their first cells
    u32* d_mask = nullptr;   // [cap_rows] the rows' masks
    if (yh_tmalloc(db, (void**)&d_chunk, std::max<u64>(n_chunks, 1) * sizeof(u64)) != hipSuccess ||
        yh_tmalloc(db, (void**)&d_mask, std::max<u64>(cap_rows, 1) * sizeof(u32)) != hipSuccess) {
        (void)hipGetLastError();
        yh_tfree(db, d_chunk); yh_tfree(db, d_mask);
        yh_set_error("device allocation failed");
        return YH_ERR_OOM;
    }
    if (n_chunks) k_matrix_cells_count<<<(u32)n_chunks, MC_THREADS, 0, st>>>(d_rows, d_n_rows, cap_rows, d_present, n_sets, db->n_refs, d_mask, d_chunk);
    k_matrix_cells_scan<<<1, MC_SCAN_THREADS, 0, st>>>(d_chunk, n_chunks, d_n_cells);
    if (n_chunks) k_matrix_cells_emit<<<(u32)n_chunks, MC_THREADS, 0, st>>>(d_rows, cap_rows, d_mask, d_med, sample_base, d_chunk, d_cells);
    const bool ok = hipGetLastError() == hipSuccess;
    yh_tfree(db, d_chunk); yh_tfree(db, d_mask);  // (the cache hands them out again behind this point of the stream)
    if (!ok) { yh_set_error("matrix cells launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

int yh_q_matrix_prevalence(yh_db* db, const yh_matrix_cell* d_cells, u64 n_cells, u32 n_sets, u32 n_samples, const u8* d_skip,
                           u32* d_prev, u64* d_denom) {
    hipStream_t st = db->stream;
    const u64 N = db->n_refs;
    if (N && hipMemsetAsync(d_prev, 0, (u64)n_sets * N * sizeof(u32), st) != hipSuccess) { yh_set_error("prevalence clear failed"); return YH_ERR_HIP; }
    if (n_samples && hipMemsetAsync(d_denom, 0, (u64)n_sets * n_samples * sizeof(u64), st) != hipSuccess) { yh_set_error("prevalence clear failed"); return YH_ERR_HIP; }
    if (n_cells == 0 || N == 0 || n_samples == 0) return YH_OK;
    // the largest power of two of slots (a key and n_sets sums each) that fits the table's share of LDS
    u32 slots_log2 = PV_MAX_SLOTS_LOG2;
    while (slots_log2 > 1 && ((u64)(sizeof(u32) + sizeof(u64) * n_sets) << slots_log2) > PV_LDS_BYTES) --slots_log2;
    const u32 lds = (u32)((sizeof(u32) + sizeof(u64) * n_sets) << slots_log2);
    const u64 tiles = (n_cells + PV_TILE - 1) / PV_TILE;
    if (tiles >> 31) { yh_set_error("too many cells for one prevalence pass"); return YH_ERR_INVALID_ARG; }
    k_matrix_prevalence<<<(u32)tiles, PV_THREADS, lds, st>>>(d_cells, n_cells, n_sets, n_samples, d_skip, N, d_prev, d_denom, slots_log2);
    if (hipGetLastError() != hipSuccess) { yh_set_error("matrix prevalence launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}

int yh_q_matrix_fill(yh_db* db, const yh_matrix_cell* d_cells, u64 n_cells, u32 bit, u32 n_samples, const u8* d_skip,
                     const int32_t* d_row_of_ref, u64 n_kept, const u64* d_denom_bit, u8* d_presence, u32* d_n_match, double* d_rel) {
    hipStream_t st = db->stream;
    const u64 n = n_kept * n_samples;
    if (n == 0) return YH_OK;
    if (hipMemsetAsync(d_presence, 0, n, st) != hipSuccess || hipMemsetAsync(d_n_match, 0, n * sizeof(u32), st) != hipSuccess ||
        (d_rel && hipMemsetAsync(d_rel, 0, n * sizeof(double), st) != hipSuccess)) {
        yh_set_error("matrix clear failed");
        return YH_ERR_HIP;
    }
    if (n_cells == 0 || db->n_refs == 0) return YH_OK;
    const u32 grid = (u32)std::min<u64>((n_cells + 255) / 256, 16384);
    k_matrix_fill<<<grid, 256, 0, st>>>(d_cells, n_cells, bit, n_samples, d_skip, db->n_refs, d_row_of_ref, n_kept, d_denom_bit,
                                        d_presence, d_n_match, d_rel);
    if (hipGetLastError() != hipSuccess) { yh_set_error("matrix fill launch failed"); return YH_ERR_HIP; }
    return YH_OK;
}
