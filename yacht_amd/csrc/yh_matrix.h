// yh_matrix.h — the organism x sample tables of a cohort (yh_matrix.hip) as yh_api.hip calls them.  Internal, like yh_common.h.
#pragma once

#include "yh_common.h"

// The rows k < min(*d_n_rows, cap_rows) with ref < N and a non-zero mask as cells in row order, and their number in
// *d_n_cells (device): three launches, no host sync (include/yacht_hip.h: yh_matrix_cells_device).  The caller has checked the
// handle, the pointers and n_sets.
int yh_q_matrix_cells(yh_db* db, const yh_batch_row* d_rows, const u32* d_n_rows, u64 cap_rows, const u8* d_present, u32 n_sets,
                      const double* d_med, u32 sample_base, yh_matrix_cell* d_cells, u64* d_n_cells);

// d_prev [n_sets][N] and d_denom [n_sets][n_samples] of n_cells cells, both cleared first (yh_matrix_prevalence_device).  The
// caller has checked the handle, the pointers and n_sets.
int yh_q_matrix_prevalence(yh_db* db, const yh_matrix_cell* d_cells, u64 n_cells, u32 n_sets, u32 n_samples, const u8* d_skip,
                           u32* d_prev, u64* d_denom);

// The three [n_kept][n_samples] matrices of one coverage bit, cleared first (yh_matrix_fill_device).  The caller has checked the
// handle, the pointers and bit.
int yh_q_matrix_fill(yh_db* db, const yh_matrix_cell* d_cells, u64 n_cells, u32 bit, u32 n_samples, const u8* d_skip,
                     const int32_t* d_row_of_ref, u64 n_kept, const u64* d_denom_bit, u8* d_presence, u32* d_n_match, double* d_rel);
