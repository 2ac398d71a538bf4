// wave_ops.h -- the wave-level primitives of the kernels (wave64), the one place they are defined.  A name says which form it is, because the
// two forms return differently:
//   butterfly (__shfl_xor)  wave_sum<T> wave_min<T> wave_max<T> group_sum<G> group_or<G> group_max<G>   the result in every lane (a VGPR)
//   DPP, whole wave         wave_sum_dpp wave_sum64_dpp wave_min_dpp                                        a wave-uniform scalar (an SGPR), no LDS crossbar traffic
//   DPP, part of a wave     quad_sum oct_sum row16_sum_of_quads                              the result in every lane of the group
// and wave_sync(), the barrier that orders one wave's own LDS traffic.
#ifndef SVT_HIP_WAVE_OPS_H
#define SVT_HIP_WAVE_OPS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// Orders the wave's own LDS traffic for the compiler: what one lane stored before this point, every lane may load after it.  The
// hardware executes a wave's LDS instructions in order, so no instruction is needed -- only the compiler must not move memory
// operations across (a lane reading what another lane wrote is invisible to its single-thread view of the program).  A workgroup
// barrier would also tie together waves that share a workgroup but not a job.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Not wave_sync(): sequentially consistent fences at workgroup scope, which the compiler turns into waits on the memory counters (tpl_kernel.hip)
__device__ __forceinline__ void wave_sync_workgroup_fences() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// ---- butterfly forms: over the G consecutive lanes of a group (a power of two) or the whole wave, the result in all of them
template <int G, typename T> __device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int G, typename T> __device__ __forceinline__ T group_or(T v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return group_sum<64>(v); }
template <typename T> __device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}
template <int G, typename T> __device__ __forceinline__ T group_max(T v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) { const T t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v) { return group_max<64>(v); }

// ---- DPP forms over the whole wave: lane 63 ends up with the result, returned to every lane as a scalar
// sum (mod 2^32): a running sum along each 16-lane row, then two row broadcasts
__device__ __forceinline__ uint32_t wave_sum_dpp(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1 (zero fill)
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);  // row_shr:8: lane 15 of every row holds the row's sum
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// a 64-bit sum in three pieces of 24 / 24 / 16 bits, none of which can overflow its 32-bit sum over 64 lanes
__device__ __forceinline__ uint64_t wave_sum64_dpp(uint64_t v) {
    const uint64_t lo = wave_sum_dpp((uint32_t)v & 0xFFFFFFu), mid = wave_sum_dpp((uint32_t)(v >> 24) & 0xFFFFFFu), hi = wave_sum_dpp((uint32_t)(v >> 48));
    return (hi << 48) + (mid << 24) + lo;
}
// minimum: a butterfly inside the 16-lane rows (min is idempotent, so the mirror patterns serve), then two row broadcasts
template <int CTRL, int ROWS> __device__ __forceinline__ uint32_t dpp_min_step(uint32_t v) {
    const uint32_t t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xF, false);
    return t < v ? t : v;
}
__device__ __forceinline__ uint32_t wave_min_dpp(uint32_t v) {
    v = dpp_min_step<0xB1, 0xF>(v);  // quad_perm [1,0,3,2]
    v = dpp_min_step<0x4E, 0xF>(v);  // quad_perm [2,3,0,1]
    v = dpp_min_step<0x141, 0xF>(v); // row_half_mirror
    v = dpp_min_step<0x140, 0xF>(v); // row_mirror
    v = dpp_min_step<0x142, 0xA>(v); // row_bcast:15 -> rows 1, 3
    v = dpp_min_step<0x143, 0xC>(v); // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- DPP forms over a part of the wave, the result in all of its lanes
__device__ __forceinline__ uint32_t quad_sum(uint32_t v) { // the 4 lanes of a quad
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true);
    return v + (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E /* quad_perm [2,3,0,1] */, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t oct_sum(uint32_t v) { // the 8 lanes of half a row
    v = quad_sum(v);
    return v + (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141 /* row_half_mirror: the other quad of the 8 */, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t row16_sum_of_quads(uint32_t v) { // v uniform inside each quad: the sum of the 4 quads of a 16-lane row
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141 /* row_half_mirror */, 0xF, 0xF, true);
    return v + (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140 /* row_mirror */, 0xF, 0xF, true);
}

} // namespace
#endif
