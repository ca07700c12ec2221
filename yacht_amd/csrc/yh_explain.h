// yh_explain.h — the per-sample-hash lookup (yh_explain.hip) as yh_api.hip calls it.  Internal, like yh_common.h.
#pragma once

#include "yh_common.h"

// flags [n_sample] (d_flags may be null: totals only) and totals [8][2] of one sample against the member table [N], enqueued
// on the handle's stream (include/yacht_hip.h: yh_explain_device).  d_abund may be null: every abundance is 1.  The caller
// has checked the handle and the pointers.
int yh_q_explain(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, const u8* d_member, u8* d_flags,
                 u64* d_totals);

// The same for a block of 1..YH_BATCH_MAX_SAMPLES samples in yh_run_batch_device's layout, sample s against the member row
// d_members + s * N: flags [total_hashes] (may be null) and totals [n_samples][8][2], one lookup launch for the block
// (yh_explain_batch_device).  The caller has checked the handle, the pointers and n_samples.
int yh_q_explain_batch(yh_db* db, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples, u64 total_hashes,
                       const u8* d_members, u8* d_flags, u64* d_totals);

// d_members [n_samples][N] from a block's compact rows and up to seven planes [n_sets][cap_rows] of their present bytes
// (yh_explain_members_rows_device).  The caller has checked the handle, the pointers, n_sets and n_samples.
int yh_q_explain_members_rows(yh_db* db, const yh_batch_row* d_rows, const u32* d_n_rows, u64 cap_rows, const u8* d_present,
                              u32 n_sets, u32 n_samples, u8* d_members);
