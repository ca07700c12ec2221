// yh_abund.h — the abundance-weighted lookup (yh_abund.hip) as yh_api.hip calls it.  Internal, like yh_common.h.
#pragma once

#include "yh_common.h"

// w_overlap / w_match [N] and, when d_med_match is not null, med_match [N] of one sample with per-hash abundances, enqueued
// on the handle's stream (include/yacht_hip.h: yh_abund_device).  The caller has checked the handle and the pointers.
int yh_q_abund(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, u64* d_w_overlap, u64* d_w_match,
               double* d_med_match);

// The same for a block of n_samples samples laid out as for yh_run_batch_device: rows [n_samples][N], every cell written by
// every call, in a number of launches that does not depend on n_samples (include/yacht_hip.h: yh_abund_batch_device).
int yh_q_abund_batch(yh_db* db, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples, u64 total_hashes,
                     u64* d_w_overlap, u64* d_w_match, double* d_med_match);
