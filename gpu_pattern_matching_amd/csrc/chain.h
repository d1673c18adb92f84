// Interface between dispatch.cpp and scan.hip: the layout of a scan workspace and the chain pipeline.
#pragma once

#include <hip/hip_runtime.h>

#include "acmatch.h"

struct acm_dfa;

namespace acm {

// Byte offsets of the areas of a scan workspace for texts up to max_text; total is what
// acm_scan_workspace_bytes answers.  The sparse pipeline has 'sparse' to itself, the LDS walk borrows
// stage1 (up to stage2), cnt (up to off) and off (up to wave_cnt1); misc is everybody's.
struct ScanLayout {
	size_t end_state, c1f, k2info, wend, probe, rflag, cnt, off, wave_cnt1, wave_cnt2, misc, stage1,
	    stage2, scan_ws, sparse;
	size_t scan_ws_bytes, total;
};
ScanLayout scan_layout(const acm_dfa *d, size_t max_text);

// words of misc: [0] last state, [1] total records, and
enum : uint32_t {
	kMiscPath = 2,       // which pipeline produced the planes (acm_scan_path_taken)
	kMiscInitDev = 4,    // carry_init_enqueue: the state to start in, device id
	kMiscInitCode = 5,   // the same as a state code of the LDS walk
};

// A scan that continues another on the device (b->d_init_plane): one thread leaves the state that
// scan ended in at misc[kMiscInitDev] and misc[kMiscInitCode], where the kernels of this scan look.
int carry_init_enqueue(const acm_dfa *d, const acm_scan_batch *b, uint32_t *misc, hipStream_t s);

// Below, l is scan_layout(d, b->n), init_dev the device id of the state to start in, and init_ptr
// null or where that id is on the device (then init_dev is not used).  The empty text: one launch.
int empty_scan_enqueue(const acm_dfa *d, const acm_scan_batch *b, const ScanLayout &l, uint32_t init_dev, const uint32_t *init_ptr,
    hipStream_t s);
// The chain pipeline for 'b' on stream s: walk, probe and resolve (speculative mode), top scan (above
// 8192 scatter blocks), scatter.  b->record_after_walk, after_walk and after_walk2 (each may be null)
// are recorded in this order behind the walk: it is the first stage and there is no second.
int chain_scan_enqueue(const acm_dfa *d, const acm_scan_batch *b, const ScanLayout &l, uint32_t init_dev, const uint32_t *init_ptr,
    hipStream_t s, hipEvent_t after_walk, hipEvent_t after_walk2);

}  // namespace acm
