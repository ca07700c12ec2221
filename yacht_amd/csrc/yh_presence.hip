// yh_presence.hip -- the presence test of a block's compact rows on the device (yh_presence_rows_device).
//
// For every row k < min(*d_n_rows, cap_rows) of a batch (yh_batch_row: sample, ref, overlap, n_excl, n_match) and every
// coverage c of the call:
//     n_cov   = (uint32_t)((double)n_excl * cov[c])           (the truncation of yh_hyp.cpp / int(x * cov))
//     p_val   = binom.cdf(n_match, n_cov, p) if n_match <= n_cov else 1
//     present = n_match >= thr[n_cov] && n_match != 0
// thr[] is the caller's table over n = 0..n_max (one yh_hyp_test over n_excl = 0..max size: the thresholds are then those of
// the host path by construction); only the p-value is device arithmetic: yh_binom.h's algorithm in double.
//
// Launch shape: one lane per (row, coverage), coverage = blockIdx.y.  The rows come in (reference, sample) order, so a wave's
// 64 lanes are mostly one reference (the same n_excl, so the same n_cov) over neighbouring samples: the tail lengths of a
// wave's lanes are alike without any sorting.  A lane reads 20 bytes and writes 13; the tail sum costs tens to thousands of
// FP64 divides per lane plus a handful of log/exp -- the kernel is bound by FP64 issue (divides, transcendentals), not
// by memory.
#include "yh_common.h"
#include "yh_binom.h"

namespace {

constexpr int PRESENCE_BLOCK = 256;

struct PresenceArgs {
    double cov[YH_PRESENCE_MAX_COVS];
    double small[16];  // stirlerr(0..15)
    double p, q, q_lo;  // q + q_lo = 1 - p exactly
    uint32_t n_max;
    uint64_t cap_rows;
};

__global__ __launch_bounds__(PRESENCE_BLOCK) void k_presence_rows(PresenceArgs a, const yh_batch_row* __restrict__ rows,
                                                                  const uint32_t* __restrict__ d_n_rows, const double* __restrict__ thr,
                                                                  double* __restrict__ p_val, uint8_t* __restrict__ present,
                                                                  uint32_t* __restrict__ n_cov_out) {
    const u64 n = min((u64)*d_n_rows, a.cap_rows);
    const u32 c = blockIdx.y;
    const double cov = a.cov[c];
    const u64 base = (u64)c * a.cap_rows;
    for (u64 k = (u64)blockIdx.x * PRESENCE_BLOCK + threadIdx.x; k < n; k += (u64)gridDim.x * PRESENCE_BLOCK) {
        const yh_batch_row r = rows[k];
        const u32 nc = (u32)((double)r.n_excl * cov);
        double pv = 1.0;
        u8 pr = 0;
        if (nc <= a.n_max) {
            if (r.n_match <= nc) pv = yh_binom::binom_cdf<double>((double)r.n_match, (double)nc, a.p, a.q, a.q_lo, a.small, 1e-22);
            pr = ((double)r.n_match >= thr[nc] && r.n_match != 0) ? 1 : 0;
        } else {
            pv = NAN;  // outside the caller's table: no decision (the caller sizes the table by the largest reference)
        }
        p_val[base + k] = pv;
        present[base + k] = pr;
        n_cov_out[base + k] = nc;
    }
}

}  // namespace

extern "C" int yh_q_presence_rows(yh_db* db, const yh_batch_row* d_rows, const u32* d_n_rows, u64 cap_rows, int ksize, double ani_thresh,
                                  const double* min_coverage, u32 n_covs, const double* d_thr, u32 n_max, double* d_p_val, u8* d_present,
                                  u32* d_n_cov) {
    if (cap_rows == 0) return YH_OK;
    PresenceArgs a{};
    for (u32 c = 0; c < n_covs; ++c) a.cov[c] = min_coverage[c];
    long double sl[16];
    yh_binom::stirlerr_table(sl);
    for (int i = 0; i < 16; ++i) a.small[i] = (double)sl[i];
    a.p = pow(ani_thresh, (double)ksize);  // (yh_hyp.cpp's p)
    a.q = yh_binom::one_minus(a.p, &a.q_lo);
    a.n_max = n_max;
    a.cap_rows = cap_rows;
    const u64 want = (cap_rows + PRESENCE_BLOCK - 1) / PRESENCE_BLOCK;
    const u32 gx = (u32)std::min<u64>(want, 4096);
    k_presence_rows<<<dim3(gx, n_covs), PRESENCE_BLOCK, 0, db->stream>>>(a, d_rows, d_n_rows, d_thr, d_p_val, d_present, d_n_cov);
    YH_HIP(hipGetLastError());
    return YH_OK;
}
