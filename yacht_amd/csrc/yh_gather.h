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
