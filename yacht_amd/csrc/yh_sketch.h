// yh_sketch.h — what yh_sketch.hip offers to the rest of the library beside the C entries of include/yacht_hip.h.  Internal, like
// yh_common.h.
#pragma once

#include "yh_common.h"

// The segmented sketch of a HOST sequence into device buffers, for a caller that goes on with the CSR on the device
// (yh_sketch.hip; yh_classify_segments): the kept pairs hashed on s_comp while the sequence goes up in pieces on s_copy
// (upload = false: the sequence is in d_seq already, one launch), then sorted and cut into d_mins / d_abund / d_off, d_totals as
// for yh_sketch_segments_device.  d_work holds yh_sketch_segments_work_bytes(cap_kept, n_seg); d_mins and d_abund cap_kept
// entries.  Nothing is synchronized.  n_seg >= 1, n_bytes >= ksize.
int yh_q_sketch_segments_hosted(const u8* seq, u64 n_bytes, u8* d_seq, const u64* d_seg_off, u32 n_seg, u32 ksize, u64 seed, u64 max_hash,
                                u64 cap_kept, void* d_work, u64* d_mins, u32* d_abund, u64* d_off, u64* d_totals, hipStream_t s_comp,
                                hipStream_t s_copy, hipEvent_t ev[2], bool upload);
