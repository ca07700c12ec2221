// yh_abund.h — the abundance-weighted lookup (yh_abund.hip) as yh_api.hip calls it.  Internal, like yh_common.h.
#pragma once

#include "yh_common.h"

// w_overlap / w_match [N] and, when d_med_match is not null, med_match [N] of one sample with per-hash abundances, enqueued
// on the handle's stream (include/yacht_hip.h: yh_abund_device).  The caller has checked the handle and the pointers.
int yh_q_abund(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, u64* d_w_overlap, u64* d_w_match,
               double* d_med_match);
