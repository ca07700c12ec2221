// yh_gather.h — the ranked minimum set cover of a sample by the candidate references (yh_gather.hip) as yh_api.hip calls it.
// Internal, like yh_common.h.
#pragma once

#include "yh_common.h"

// Rows [<= cap_rows], *n_rows, *more (both HOST) and, when d_owner is not null, owner [n_sample] of one sample against the
// candidate table [N] (include/yacht_hip.h: yh_gather_device).  d_abund may be null: every abundance is 1.  Enqueued on the
// handle's stream, which it synchronizes once per YH_GATHER_ROUNDS_PER_SYNC rounds.  The caller has checked the handle, the
// pointers, min_hits >= 1 and n_sample < 2^32.
int yh_q_gather(yh_db* db, const u64* d_sample, const u32* d_abund, u64 n_sample, const u8* d_cand, u32 min_hits,
                yh_gather_row* d_rows, u64 cap_rows, u32* d_owner, u64* n_rows, int* more);

// The same for a block of samples (include/yacht_hip.h: yh_gather_batch_device): rows [n_samples][cap_rows], d_n_rows and d_more
// [n_samples] (both DEVICE), owner [total_hashes] or null.  Sample s's candidates are (d_members[s * N + j] & cand_mask) != 0.
// Enqueued on the handle's stream, min(cap_rows, N) + 1 rounds of two launches; it never synchronizes.  The caller has checked
// the handle, the pointers, n_samples, cand_mask != 0, min_hits >= 1, cap_rows <= YH_GATHER_BATCH_MAX_ROWS and total_hashes < 2^32.
int yh_q_gather_batch(yh_db* db, const u64* d_samples, const u64* d_soff, const u32* d_abund, u32 n_samples, u64 total_hashes,
                      const u8* d_members, u8 cand_mask, u32 min_hits, yh_gather_row* d_rows, u64 cap_rows, u32* d_owner,
                      u32* d_n_rows, u8* d_more);
