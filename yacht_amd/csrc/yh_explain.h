// yh_explain.h — the per-sample-hash lookup (yh_explain.hip) as yh_api.hip calls it.  Internal, like yh_common.h.
#pragma once

#include "yh_common.h"

// flags [n_sample] (d_flags may be null: totals only) and totals [8][2] of one sample against the member table [N], enqueued
// on the handle's stream (include/yacht_hip.h: yh_explain_device).  d_abund may be null: every abundance is 1.  The caller
// has checked the handle and the pointers.
int yh_q_explain(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, const u8* d_member, u8* d_flags,
                 u64* d_totals);
