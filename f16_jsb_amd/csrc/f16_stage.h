// f16_stage.h -- how a block of any env kernel is shaped and gets the table blob into LDS: BLOCK,
// the compiler-visible vector-memory waits (VM_DRAIN, VM_WAIT), the LDS-DMA moves (dma16, dma4)
// and stage_tables. Device code only. Needs f16_tables.h (the blob) by way of f16_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include "f16_device.h"

using namespace f16;

#ifndef BLOCK
#define BLOCK 256
#endif

// Wait for every outstanding vector-memory operation (s_waitcnt vmcnt(0)) as the compiler's
// own wait: its wait-insertion pass then knows the LDS-DMA issued before is retired. (An
// inline-asm s_waitcnt is opaque to that pass: it kept treating the fresh-frame DMA into the
// staging area as pending and put another vmcnt(0) before the slot staging's LDS writes --
// which on CDNA also waits for every state store issued in between.) The empty asm statements
// keep the compiler from moving memory operations across it.
#define VM_DRAIN()                          \
  do {                                      \
    asm volatile("" ::: "memory");          \
    __builtin_amdgcn_s_waitcnt(0x0F70);     \
    asm volatile("" ::: "memory");          \
  } while (0)
// ... and for all but the youngest k of them (s_waitcnt vmcnt(k), k < 64 a constant; gfx9
// encoding: vmcnt in bits 3:0 and 15:14, expcnt 6:4 and lgkmcnt 11:8 left at "no wait")
#define VM_WAIT(k)                                                                      \
  do {                                                                                  \
    static_assert((k) >= 0 && (k) < 64, "vmcnt is a 6-bit count");                      \
    asm volatile("" ::: "memory");                                                      \
    __builtin_amdgcn_s_waitcnt(0x0F70 | ((k) & 15) | ((((k) >> 4) & 3) << 14));         \
    asm volatile("" ::: "memory");                                                      \
  } while (0)

// LDS-DMA of 16 B per lane: lane i's 16 bytes land at lds + 16*i (gfx950 global_load_lds_dwordx4)
__device__ __forceinline__ void dma16(const float* g, float* lds) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                   (void __attribute__((address_space(3)))*)lds, 16, 0, 0);
}
// ... and of 4 B per lane (lane i's dword lands at lds + 4*i)
__device__ __forceinline__ void dma4(const float* g, float* lds) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                   (void __attribute__((address_space(3)))*)lds, 4, 0, 0);
}
// Table blob -> LDS by LDS-DMA (no VGPRs, no wait at issue): the caller issues its other
// loads behind it and completes the staging with one s_waitcnt vmcnt(0) + barrier.
__device__ __forceinline__ void stage_tables_issue(float* sT) {
  constexpr int NP = F16_BLOB_FLOATS / 4;  // 16-byte pieces (the generator pads the blob)
  static_assert(F16_BLOB_FLOATS % 4 == 0, "blob must be whole 16-byte pieces");
  const int wave_base = threadIdx.x & ~63;
  // stride BLOCK, not blockDim.x: every kernel that stages the tables launches BLOCK threads, and
  // blockDim.x is a load from the implicit kernel arguments -- the wait for it held the DMA (and
  // the state loads behind it) until the whole argument block had arrived
  for (int r = 0; r < NP; r += BLOCK) {
    const int piece = r + threadIdx.x;
    if (piece < NP) dma16(F16_BLOB_INIT + 4 * piece, sT + 4 * (r + wave_base));
  }
}
__device__ __forceinline__ void stage_tables(float* sT) {
  stage_tables_issue(sT);
  VM_DRAIN();
  __syncthreads();
}
