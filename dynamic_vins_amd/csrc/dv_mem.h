// dv_mem.h — what a DV_MEM_* memory kind means to the library.  Plain C++ (no HIP): the *_host.h headers include it.
#pragma once
#include "../../include/dvins.h"

static inline bool dv_mem_known(int mem) { return mem == DV_MEM_HOST || mem == DV_MEM_DEVICE || mem == DV_MEM_PINNED; }
// The two policies of the staging rule (dv_stage_rows, dv_ctx.h): which of a caller's arrays the kernels read where they lie.  Every other kind is copied.
static inline bool dv_in_place_device(int mem) { return mem == DV_MEM_DEVICE; }                                      // pinned memory is copied like pageable memory
static inline bool dv_in_place_device_or_pinned(int mem) { return mem == DV_MEM_DEVICE || mem == DV_MEM_PINNED; }      // pinned + mapped host memory is device-addressable
