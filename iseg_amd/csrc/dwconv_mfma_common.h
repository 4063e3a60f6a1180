// Pieces shared by the matrix-core depthwise kernels (dwconv_mfma.hip: forward / data gradient, dwconv_wgrad_mfma.hip: weight gradient):
// operand types of v_mfma_f32_4x4x4_16b_bf16, LDS-DMA pointer types, the raw barrier and the transposing LDS read.
#pragma once
#include "common.h"

namespace dwm {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* glb_ptr;

// ds_read_b64_tr_b16: inside a 16-lane group, lane 4 k + p supplies the address of four consecutive 16-bit elements (elements 4 p .. 4 p + 3 of
// row k); afterwards lane i of the group holds element i of rows 0 .. 3.  Needs a full EXEC mask; the caller waits (lgkmcnt) before using `out`.
__device__ __forceinline__ void lds_read_tr16_b64(u32x2_t& out, unsigned addr) {
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(out) : "v"(addr) : "memory");
}

}  // namespace dwm

// Every LDS access that may run while an LDS-DMA (global_load_lds) is in flight is inline assembly: hipcc has no alias information between an LDS
// access it can see and the DMA, and would put s_waitcnt vmcnt(0) in front of it.  The waits are written out; barriers are raw s_barrier
// (__syncthreads() carries a fence that drains vmcnt as well).
#define DWM_BARRIER()                                       \
    do {                                                    \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
        __builtin_amdgcn_s_barrier();                       \
        asm volatile("" ::: "memory");                      \
    } while (0)
