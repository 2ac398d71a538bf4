// lds_dma.h -- direct-to-LDS loads (global_load_lds_dwordx4) for one-wave workgroups, the one place they are defined.  Such a load has no
// register destination: lane l's 16 bytes go from ITS OWN global address to LDS byte (wave-uniform base) + 16 * l.  It counts on vmcnt like
// any global load, and nothing but the issuing wave's own wait orders a later LDS read behind it -- lds_dma_wait(), which the caller
// places in front of the first read of a destination (a wave is the whole workgroup here, so no barrier is involved).
//
// Two rules the call sites keep (the hardware orders neither):
//   1. a plain LDS store to bytes that a direct load will overwrite has retired before that load is issued (lds_dma_after_stores());
//   2. two direct loads in flight never share destination bytes.
// A lane whose predicate is false is switched off in the exec mask and writes nothing: copies mask the lanes beyond their end, they
// never clamp them onto the last vector and never write past the destination.
//
// Source alignment: tools/ubench/lds_dma_phase.hip (profiles/r05_lds_dma_phase.txt) checks every source byte phase 0..15 against row
// strides = 0, 4, 8, 12 (mod 16), and lanes switched off at the end and in the middle of an instruction: all exact, nothing written
// beside the destination.  The LDS destination of every call is 16-byte aligned.
#ifndef SVT_HIP_LDS_DMA_H
#define SVT_HIP_LDS_DMA_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// lane l: 16 bytes from g (this lane's address, any byte alignment the phase table allows) to lds[off + 16 * l]; `off` is wave-uniform
// and a multiple of 16.  `lds` is the wave's LDS slice.
__device__ __forceinline__ void lds_dma_load16(const uint8_t *g, uint8_t *lds, uint32_t off) {
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(g)),
                                     (__attribute__((address_space(3))) void *)(lds + off), 16, 0, 0);
}

// the wave: lds[off + 16 * i] = 16 bytes at g + 16 * i, i in [0, n); n is wave-uniform
__device__ __forceinline__ void lds_dma_copy(const uint8_t *g, uint8_t *lds, uint32_t off, int n) {
    const int lane = threadIdx.x & 63;
    for (int b = 0; b < n; b += 64) // uniform
        if (b + lane < n) lds_dma_load16(g + (size_t)(b + lane) * 16, lds, off + (uint32_t)b * 16);
}

// the wave: a 2-D window of `rows` rows of vec_per_row 16-byte vectors, row r at g + r * stride, to lds[off ..) row after row without
// gaps (vector k = r * vec_per_row + c at off + 16 * k).  All of it is issued before the caller's one wait.  (k stays below 2^20: the
// float quotient is exact.)
__device__ __forceinline__ void lds_dma_window(const uint8_t *g, uint32_t stride, int vec_per_row, int rows, uint8_t *lds, uint32_t off) {
    const int   lane = threadIdx.x & 63, nvec = vec_per_row * rows;
    const float rcp  = __builtin_amdgcn_rcpf((float)vec_per_row);
    for (int b = 0; b < nvec; b += 64) { // uniform
        const int k = b + lane;
        if (k < nvec) {
            const int row = (int)(((float)k + 0.5f) * rcp), c = k - row * vec_per_row;
            lds_dma_load16(g + ((uint32_t)row * stride + (uint32_t)c * 16), lds, off + (uint32_t)b * 16); // (a window spans far less than 4 GiB)
        }
    }
}

// rule 1: the wave's earlier LDS stores have retired (and the compiler keeps them in front)
__device__ __forceinline__ void lds_dma_after_stores() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0); vmcnt and expcnt left alone (gfx9 encoding)
    __builtin_amdgcn_wave_barrier();
}

// every direct load the wave has issued has landed; LDS reads after this see it
__device__ __forceinline__ void lds_dma_wait() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0); lgkmcnt and expcnt left alone (gfx9 encoding: vmcnt = bits 3:0 and 15:14)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace
#endif
